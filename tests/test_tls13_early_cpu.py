"""CPU-side checks of the resumed-handshake batches (include/tlsrec.h:
tlsrec_tls13_batch_psk_binder, tlsrec_tls13_keytab_derive_early,
tlsrec_tls13_batch_ticket_psk): the hashlib checker of the GPU tests chained
through the reference's RFC 8448 resumption vectors, the entry points and the
connection layout, and the argument errors the calls decide on the host before
any launch.  No test here needs a GPU."""
import ctypes
import json
import os
import re

import mbedtls_amd as M
from mbedtls_amd import _abi
from mbedtls_amd import keysched as K
from tests import tls13_early_ref as E
from tests import tls13_ref as R

HERE = os.path.dirname(__file__)
KEYS = json.load(open(os.path.join(HERE, "golden", "tls13_keys.json")))
G = json.load(open(os.path.join(HERE, "golden", "tls13_handshake.json")))
HEADER = os.path.join(os.path.dirname(HERE), "include", "tlsrec.h")
X = bytes.fromhex
BAD, UNA = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
SHA512 = 0x0200000b

CALLS = ["tlsrec_tls13_batch_psk_binder", "tlsrec_tls13_keytab_derive_early", "tlsrec_tls13_batch_ticket_psk"]


def test_checker_chains_the_rfc8448_resumption_vectors():
    """test_suite_ssl.data:2681 (the "resumption" Expand-Label) gives the PSK of
    :2850 (the binder), whose Early Secret is the secret of :2768 (c e traffic,
    e exp master)"""
    t = [v for v in KEYS["expand_label"] if v["label"] == "resumption"]
    assert len(t) == 1 and t[0]["where"] == "test_suite_ssl.data:2681" and t[0]["ctx"] == "0000"
    psk = E.ticket_psk(t[0]["hash"], X(t[0]["secret"]), X(t[0]["ctx"]))
    assert psk.hex() == t[0]["expected"] == "4ecd0eb6ec3b4d87f5d6028f922ca4c5851a277fd41311c9e62d2c9492e1c4f3"
    b, e = G["psk_binder"][0], G["early_secrets"][0]
    assert b["psk"] == psk.hex() and b["hash"] == e["hash"] == t[0]["hash"] == "sha256"
    assert b["psk_type"] == "MBEDTLS_SSL_TLS1_3_PSK_RESUMPTION"
    st = E.early_stage("sha256", psk, True, X(b["transcript"]), X(e["transcript"]), 16)
    assert st["binder"].hex() == b["binder"] == "3add4fb2d8fdf822a0ca3cf7678ef5e88dae990141c5924d57bb6fa31b9e5f9d"
    assert st["early"].hex() == e["secret"] == "9b2188e9b2fc6d64d71dc329900e20bb41915000f678aa839cbb797cb7d8332c"
    assert st["c_e"].hex() == e["client_early_traffic_secret"]
    assert st["e_exp"].hex() == e["early_exporter_master_secret"]
    assert st["keys"] == R.traffic_keys("sha256", st["c_e"], 16) and [len(x) for x in st["keys"]] == [16, 12]
    # an external PSK takes the other label: another binder, the same early secrets
    ext = E.early_stage("sha256", psk, False, X(b["transcript"]), X(e["transcript"]), 16)
    assert ext["binder"] != st["binder"] and ext["binder"] == R.psk_binder("sha256", psk, False, X(b["transcript"]))
    assert (ext["c_e"], ext["e_exp"]) == (st["c_e"], st["e_exp"])


def test_checker_ticket_psk_is_the_expand_label_of_the_nonce():
    for hname in ("sha256", "sha384"):
        rm = bytes(range(R.HLEN[hname]))
        for n in (0, 1, 32):
            nonce = bytes(0x80 + k for k in range(n))
            got = E.ticket_psk(hname, rm, nonce)
            assert got == R.expand_label(hname, rm, b"resumption", nonce, R.HLEN[hname]) and len(got) == R.HLEN[hname]
        assert E.ticket_psk(hname, rm, b"\x00") != E.ticket_psk(hname, rm, b"")


def test_library_exports_and_layout():
    L = M.load()
    for n in CALLS + ["tlsrec__tls13_stage_early_keys"]:
        assert hasattr(L, n), n
    c = _abi.CTls13PskConn
    assert ctypes.sizeof(c) == 144 == K.PSK_CONN_BYTES
    assert (c.psk.offset, c.binder_transcript.offset, c.hello_transcript.offset) == (0, 48, 96)
    assert K.TICKET_NONCE_BYTES == 32


def _params(proto):
    return [p.strip() for p in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]


def test_header_and_bindings_agree():
    src = open(HEADER).read()
    m = re.search(r"typedef struct tlsrec_tls13_psk_conn \{(.*?)\} tlsrec_tls13_psk_conn;", src, flags=re.S)
    assert m, "include/tlsrec.h lacks tlsrec_tls13_psk_conn"
    fields = re.findall(r"uint8_t\s+(\w+)\[(\d+)\];", m.group(1))
    assert fields == [(n, str(ctypes.sizeof(t))) for n, t in _abi.CTls13PskConn._fields_]
    kinds = {ctypes.c_int: "int", ctypes.c_uint32: "uint32_t"}
    for name in CALLS:
        m = re.search(r"\bint " + name + r"\((.*?)\);", src, flags=re.S)
        assert m, name
        res, args = _abi.SIGNATURES[name]
        params = _params(m.group(1))
        assert res is ctypes.c_int and len(params) == len(args), name
        for p, a in zip(params, args):
            if a is ctypes.c_void_p:
                assert "*" in p, (name, p)
            else:
                assert "*" not in p and p.split()[0] == kinds[a], (name, p)


def test_table_less_argument_errors_need_no_gpu():
    """every check of tlsrec_tls13_batch_psk_binder and tlsrec_tls13_batch_ticket_psk,
    in the header's order; p is never dereferenced: every call returns before a launch"""
    L = M.load()
    p = 0x1000
    pb, tk = L.tlsrec_tls13_batch_psk_binder, L.tlsrec_tls13_batch_ticket_psk
    res, ext = K.PSK_RESUMPTION, K.PSK_EXTERNAL
    for alg in (0, SHA512):
        for count in (0, 4):
            assert pb(alg, 32, res, p, p, p, p, count, None) == BAD
            assert tk(alg, 32, p, p, p, count, None) == BAD
            assert tk(alg, 33, p, p, p, count, None) == BAD            # BAD_INPUT_DATA before FEATURE_UNAVAILABLE
    for a in (K.ALG_SHA_256, K.ALG_SHA_384):
        # the binder
        assert pb(a, 32, res, None, p, p, p, 4, None) == BAD             # conns
        assert pb(a, 32, res, p, p, p, None, 4, None) == BAD             # offered without match
        assert pb(a, 32, res, p, None, p, p, 4, None) == BAD             # match without offered
        assert pb(a, 32, res, p, p, p, None, 0, None) == BAD             # ... whatever the count
        assert pb(a, 32, res, p, None, None, p, 0, None) == BAD
        assert pb(a, 32, ext, p, None, None, None, 4, None) == BAD       # nothing to write
        for n in (0, 49, 0xFFFFFFFF):
            assert pb(a, n, res, p, p, p, p, 4, None) == BAD
            assert pb(a, n, res, p, p, p, p, 0, None) == BAD
            assert pb(a, n, ext, p, None, p, None, 0, None) == BAD
        for n in (1, 48):
            assert pb(a, n, res, p, p, p, p, 0, None) == 0               # count == 0 after the checks
            assert pb(a, n, ext, p, None, p, None, 0, None) == 0
            assert pb(a, n, res, p, p, None, p, 0, None) == 0
            assert pb(a, n, 7, None, None, None, None, 0, None) == 0
        # the ticket PSK
        assert tk(a, 32, None, p, p, 4, None) == BAD
        assert tk(a, 32, p, None, p, 4, None) == BAD
        assert tk(a, 32, p, p, None, 4, None) == BAD
        assert tk(a, 33, None, p, p, 4, None) == BAD                     # BAD_INPUT_DATA before FEATURE_UNAVAILABLE
        for n in (33, 64, 255, 0xFFFFFFFF):
            assert tk(a, n, p, p, p, 4, None) == UNA
            assert tk(a, n, p, p, p, 0, None) == UNA                     # ... and before count == 0
            assert tk(a, n, None, None, None, 0, None) == UNA
        for n in (0, 1, 32):
            assert tk(a, n, p, p, p, 0, None) == 0
            assert tk(a, n, None, None, None, 0, None) == 0


def test_keytab_call_without_a_table_needs_no_gpu():
    """a NULL table is BAD_INPUT_DATA before anything else is looked at (the
    checks that need a table are in tests/test_tls13_early_gpu.py)"""
    L = M.load()
    p = 0x1000
    for f in (L.tlsrec_tls13_keytab_derive_early, L.tlsrec__tls13_stage_early_keys):
        f.restype, f.argtypes = _abi.SIGNATURES["tlsrec_tls13_keytab_derive_early"]
        for cipher in (M.CIPHER_AES_128_GCM, 0):
            for count in (0, 4):
                for psk_len in (0, 32, 49):
                    assert f(None, 0, count, cipher, psk_len, K.PSK_RESUMPTION, p, p, p, p, p, p, None) == BAD
                    assert f(None, 0, count, cipher, psk_len, K.PSK_EXTERNAL, p, None, p, None, p, None, None) == BAD
