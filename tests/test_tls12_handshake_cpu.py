"""CPU-side checks of the TLS 1.2 handshake batches (include/tlsrec.h:
tlsrec_tls12_batch_compute_master, tlsrec_tls12_batch_verify_data,
tlsrec_tls12_calc_finished, tlsrec_tls12_psk_premaster): the connection layout,
every argument error the calls decide on the host before any launch, in the
header's order, the host-only PSK premaster, and the checker of the GPU tests
(tests/tls12_hs_ref.py) pinned to the reference's PRF vectors and to the
existing key-block split.  No test here needs a GPU."""
import ctypes
import json
import os
import re

import pytest

import mbedtls_amd as M
from mbedtls_amd import _abi
from mbedtls_amd import tls12 as T
from tests import tls12_hs_ref as H
from tests.prng import prng_bytes
from tests.tls12_ref import p_hash, split_key_block

HERE = os.path.dirname(__file__)
G = json.load(open(os.path.join(HERE, "golden", "tls12_prf.json")))
HEADER = os.path.join(os.path.dirname(HERE), "include", "tlsrec.h")
X = bytes.fromhex
BAD, UNA, SMALL = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE, _abi.ERR_SSL_BUFFER_TOO_SMALL
PRF = {"sha256": T.PRF_SHA256, "sha384": T.PRF_SHA384}
CALLS = ["tlsrec_tls12_batch_compute_master", "tlsrec_tls12_batch_verify_data", "tlsrec_tls12_calc_finished",
         "tlsrec_tls12_psk_premaster"]


def test_layout_of_the_premaster_connection():
    c = _abi.CTls12PmsConn
    assert ctypes.sizeof(c) == 240 == T.PMS_CONN_BYTES == H.PMS_CONN
    assert (c.premaster.offset, c.randbytes.offset, c.session_hash.offset) == (0, 128, 192)
    assert (c.premaster.size, c.randbytes.size, c.session_hash.size) == (128, 64, 48)
    assert ctypes.sizeof(_abi.CTls12Conn) == 112 == T.CONN_BYTES == H.CONN
    L = M.load()
    for n in CALLS:
        assert hasattr(L, n) and n in _abi.SIGNATURES, n
    for n in ("tls12_batch_compute_master", "tls12_batch_verify_data", "tls12_calc_finished", "tls12_psk_premaster",
              "PMS_CONN_BYTES"):
        assert n in T.__all__ and hasattr(T, n), n


def test_header_and_bindings_agree():
    src = open(HEADER).read()
    m = re.search(r"typedef struct tlsrec_tls12_pms_conn \{(.*?)\} tlsrec_tls12_pms_conn;", src, flags=re.S)
    assert m, "include/tlsrec.h lacks tlsrec_tls12_pms_conn"
    fields = re.findall(r"uint8_t\s+(\w+)\[(\d+)\];", m.group(1))
    assert fields == [(n, str(ctypes.sizeof(t))) for n, t in _abi.CTls12PmsConn._fields_]
    kinds = {ctypes.c_int: "int", ctypes.c_uint32: "uint32_t", ctypes.c_size_t: "size_t"}
    for name in CALLS:
        m = re.search(r"\bint " + name + r"\((.*?)\);", src, flags=re.S)
        assert m, name
        res, args = _abi.SIGNATURES[name]
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert res is ctypes.c_int and len(params) == len(args), name
        for p, a in zip(params, args):
            if a is ctypes.c_void_p:
                assert "*" in p or "[" in p, (name, p)
            else:
                assert "*" not in p and p.split()[0] == kinds[a], (name, p)


def test_compute_master_argument_errors_need_no_gpu():
    """the header's order: the prf; conns or out NULL with count != 0, then pms_len == 0; pms_len > 128;
    count == 0.  p is never dereferenced: every call returns before a launch"""
    fn = M.load().tlsrec_tls12_batch_compute_master
    p = 0x1000
    for prf in (T.PRF_NONE, 3, -1, 0x02000009):
        for pms_len in (0, 48, 129):
            for count in (0, 4):
                for ems in (0, 1):
                    assert fn(prf, pms_len, ems, p, p, count, None) == UNA
                    assert fn(prf, pms_len, ems, None, None, count, None) == UNA     # the prf before the NULL arrays
    for prf in PRF.values():
        for ems in (0, 1, 7):
            for pms_len in (0, 48, 129):
                assert fn(prf, pms_len, ems, None, p, 4, None) == BAD                # conns
                assert fn(prf, pms_len, ems, p, None, 4, None) == BAD                # out; both before pms_len > 128
            for count in (0, 4):
                assert fn(prf, 0, ems, p, p, count, None) == BAD                     # pms_len == 0, whatever the count
            assert fn(prf, 0, ems, None, None, 0, None) == BAD
            for pms_len in (129, 256, 384, 0xFFFFFFFF):                              # the FFDH premasters
                assert fn(prf, pms_len, ems, p, p, 4, None) == UNA
                assert fn(prf, pms_len, ems, p, p, 0, None) == UNA                   # ... before count == 0
                assert fn(prf, pms_len, ems, None, None, 0, None) == UNA
            for pms_len in (1, 48, 66, 118, 128):
                assert fn(prf, pms_len, ems, p, p, 0, None) == 0                     # count == 0 after the checks
                assert fn(prf, pms_len, ems, None, None, 0, None) == 0
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_batch_compute_master(T.PRF_SHA256, 129, False, p, p, 4)
    assert e.value.code == UNA


def test_verify_data_argument_errors_need_no_gpu():
    """the header's order: the prf; `from`; conns or transcripts NULL with count != 0; only one of offered and
    match; verify and match both NULL with count != 0; count == 0"""
    fn = M.load().tlsrec_tls12_batch_verify_data
    p = 0x1000
    cli, srv = T.IS_CLIENT, T.IS_SERVER
    for prf in (T.PRF_NONE, 3, -1):
        for frm in (cli, srv, 2):
            for count in (0, 4):
                assert fn(prf, frm, p, p, p, p, p, count, None) == UNA
                assert fn(prf, frm, None, None, p, None, None, count, None) == UNA   # the prf before everything else
    for prf in PRF.values():
        for frm in (2, -1, 256):
            for count in (0, 4):
                assert fn(prf, frm, p, p, p, p, p, count, None) == BAD
        for frm in (cli, srv):
            assert fn(prf, frm, None, p, p, p, p, 4, None) == BAD                    # conns
            assert fn(prf, frm, p, None, p, p, p, 4, None) == BAD                    # transcripts
            assert fn(prf, frm, p, p, p, p, None, 4, None) == BAD                    # offered without match
            assert fn(prf, frm, p, p, None, p, p, 4, None) == BAD                    # match without offered
            assert fn(prf, frm, p, p, p, p, None, 0, None) == BAD                    # ... whatever the count
            assert fn(prf, frm, p, p, None, None, p, 0, None) == BAD
            assert fn(prf, frm, p, p, None, None, None, 4, None) == BAD              # nothing to write
            assert fn(prf, frm, p, p, p, p, p, 0, None) == 0                         # count == 0 after the checks
            assert fn(prf, frm, p, p, p, None, p, 0, None) == 0
            assert fn(prf, frm, p, p, None, p, None, 0, None) == 0
            assert fn(prf, frm, None, None, None, None, None, 0, None) == 0
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_batch_verify_data(T.PRF_SHA256, 2, p, p, p, p, p, 4)
    assert e.value.code == BAD


def test_calc_finished_argument_errors_need_no_gpu():
    fn = M.load().tlsrec_tls12_calc_finished
    out = ctypes.create_string_buffer(b"\xa5" * 12, 12)
    m, t = bytes(48), bytes(48)
    for prf in (T.PRF_NONE, 3, -1):
        assert fn(prf, m, t, T.IS_CLIENT, out) == UNA
        assert fn(prf, None, None, 2, None) == UNA
    for prf in PRF.values():
        assert fn(prf, m, t, 2, out) == BAD
        assert fn(prf, None, t, T.IS_CLIENT, out) == BAD
        assert fn(prf, m, None, T.IS_SERVER, out) == BAD
        assert fn(prf, m, t, T.IS_SERVER, None) == BAD
    assert out.raw == b"\xa5" * 12
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_calc_finished(T.PRF_SHA256, bytes(48), bytes(48), T.IS_CLIENT)       # a SHA-384 digest under SHA-256
    assert e.value.code == BAD


@pytest.mark.parametrize("other_len", [None, 32, 66])
def test_psk_premaster(other_len):
    """plain PSK, a 32-byte and a 66-byte other secret (ECDHE-PSK over x25519 / secp521r1), against the checker"""
    for k, psk_len in enumerate((1, 16, 32, 48)):
        psk = prng_bytes(0x9500 + k, psk_len)
        other = None if other_len is None else prng_bytes(0x9510 + k, other_len)
        want = H.psk_premaster(psk, other)
        assert len(want) == 4 + (psk_len if other is None else other_len) + psk_len
        assert T.tls12_psk_premaster(psk, other) == want
        if other is None:
            assert want == psk_len.to_bytes(2, "big") + bytes(psk_len) + psk_len.to_bytes(2, "big") + psk
        # one byte short: BUFFER_TOO_SMALL, nothing written; room to spare: only the premaster is written
        fn = M.load().tlsrec_tls12_psk_premaster
        buf = ctypes.create_string_buffer(b"\xa5" * 160, 160)
        olen = ctypes.c_size_t(7)
        args = (other, 0 if other is None else len(other), psk, len(psk))
        assert fn(*args, buf, len(want) - 1, ctypes.byref(olen)) == SMALL
        assert buf.raw == b"\xa5" * 160 and olen.value == 7
        assert fn(*args, buf, 160, ctypes.byref(olen)) == 0
        assert olen.value == len(want) and buf.raw == want + b"\xa5" * (160 - len(want))
    assert 4 + 66 + 48 == 118 == len(H.psk_premaster(bytes(48), bytes(66)))       # the longest form of the reference


def test_psk_premaster_argument_errors():
    fn = M.load().tlsrec_tls12_psk_premaster
    buf = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    olen = ctypes.c_size_t(7)
    psk = bytes(range(16))
    assert fn(None, 0, None, 16, buf, 64, ctypes.byref(olen)) == BAD
    assert fn(None, 0, psk, 16, None, 64, ctypes.byref(olen)) == BAD
    assert fn(None, 0, psk, 16, buf, 64, None) == BAD
    assert fn(None, 0, psk, 0, buf, 64, ctypes.byref(olen)) == BAD
    assert fn(None, 0, psk, 0, buf, 0, ctypes.byref(olen)) == BAD                  # BAD_INPUT_DATA before too small
    assert fn(None, 8, psk, 16, buf, 64, ctypes.byref(olen)) == BAD                # a length without its bytes
    assert fn(None, 0, psk, 16, buf, 35, ctypes.byref(olen)) == SMALL
    assert fn(None, 0, psk, 16, buf, 0, ctypes.byref(olen)) == SMALL
    assert buf.raw == b"\xa5" * 64 and olen.value == 7
    for size, code in ((35, SMALL), (0, SMALL)):
        with pytest.raises(T.KeyScheduleError) as e:
            T.tls12_psk_premaster(psk, None, out_size=size)
        assert e.value.code == code


def test_checker_reproduces_reference_vectors():
    """the yardstick is itself pinned: its PRF gives the reference's own answers (test_suite_ssl.data:2857, :2861),
    and master / verify_data are that PRF under their labels"""
    for v in G["vectors"]:
        want = X(v["expected"])
        assert H.prf(v["prf"], X(v["secret"]), v["label"].encode() + X(v["random"]), len(want)) == want
    for hname, hl in H.HLEN.items():
        pms, rb, sh = prng_bytes(1, 48), prng_bytes(2, 64), prng_bytes(3, hl)
        assert H.master(hname, pms, rb) == p_hash(hname, pms, b"master secret" + rb, 48)
        assert H.master(hname, pms, rb, sh) == p_hash(hname, pms, b"extended master secret" + sh, 48)
        assert H.master(hname, pms, rb) != H.master(hname, pms, rb, sh)
        ms = H.master(hname, pms, rb)
        for frm, label in ((0, b"client finished"), (1, b"server finished")):
            assert H.verify_data(hname, ms, sh, frm) == p_hash(hname, ms, label + sh, 12)
        assert H.verify_data(hname, ms, sh, 0) != H.verify_data(hname, ms, sh, 1)


@pytest.mark.parametrize("hname", sorted(PRF))
def test_checker_output_feeds_the_key_expansion(hname):
    """the swap: the checker's tlsrec_tls12_conn, cut as the derive calls read it and split by the existing
    key-block split, gives what P_hash("key expansion", server_random || client_random) gives"""
    cipher = M.CIPHER_AES_128_GCM if hname == "sha256" else M.CIPHER_AES_256_GCM
    kl = M.KEYLEN[cipher]
    for ems in (False, True):
        pc = prng_bytes(0x9600 + ems, H.PMS_CONN)
        cli, srv = pc[128:160], pc[160:192]
        assert cli != srv
        out = H.conn_out(hname, pc, 48, ems)
        assert len(out) == H.CONN and out[48:] == srv + cli == H.swap(pc[128:192])
        ms = out[:48]
        assert ms == p_hash(hname, pc[:48], (b"extended master secret" + pc[192:192 + H.HLEN[hname]]) if ems
                            else (b"master secret" + cli + srv), 48)
        blk = p_hash(hname, ms, b"key expansion" + srv + cli, 2 * kl + 8)
        assert T.tls12_split_key_block(cipher, blk) == split_key_block(blk, kl, 4)
        assert blk != p_hash(hname, ms, b"key expansion" + cli + srv, 2 * kl + 8)     # the unswapped order differs
