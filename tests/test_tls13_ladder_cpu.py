"""CPU-side checks of the TLS 1.3 ladder (include/tlsrec.h, "the rest of the TLS
1.3 ladder"): the hashlib checker of the GPU tests against the reference's own
vectors, the new entry points and layouts, the constants the batch kernels
take, and the argument errors the batch calls decide before they touch a
device.  No test here needs a GPU."""
import ctypes
import hashlib
import json
import os

import pytest

import mbedtls_amd as M
from mbedtls_amd import _abi
from mbedtls_amd import keysched as K
from tests import tls13_ref as R

HERE = os.path.dirname(__file__)
KEYS = json.load(open(os.path.join(HERE, "golden", "tls13_keys.json")))
G = json.load(open(os.path.join(HERE, "golden", "tls13_handshake.json")))
X = bytes.fromhex
ALG = {"sha256": K.ALG_SHA_256, "sha384": K.ALG_SHA_384}
BAD, UNA = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE

NEW = ["tlsrec_tls13_derive_early_secrets", "tlsrec_tls13_derive_handshake_secrets",
       "tlsrec_tls13_derive_application_secrets", "tlsrec_tls13_derive_resumption_master_secret",
       "tlsrec_tls13_calc_finished", "tlsrec_tls13_create_psk_binder", "tlsrec_tls13_keytab_derive_handshake",
       "tlsrec_tls13_keytab_derive_application", "tlsrec_tls13_batch_verify_data", "tlsrec_tls13_batch_derive_secret",
       "tlsrec__tls13_stage_hs_keys", "tlsrec__tls13_stage_app_keys"]


def test_checker_reproduces_the_existing_vectors():
    assert len(KEYS["derive_secret"]) >= 10 and len(KEYS["evolve"]) == 3
    for v in KEYS["derive_secret"]:
        got = R.derive_secret(v["hash"], X(v["secret"]), v["label"].encode(), X(v["ctx"]), bool(v["ctx_hashed"]))
        assert got[:v["len"]].hex() == v["expected"] and v["len"] == R.HLEN[v["hash"]], v["where"]
    for v in KEYS["evolve"]:
        assert R.evolve(v["hash"], X(v["secret"]) or None, X(v["input"]) or None).hex() == v["expected"], v["where"]
    for v in KEYS["expand_label"]:
        assert R.expand_label(v["hash"], X(v["secret"]), v["label"].encode(), X(v["ctx"]), v["len"]).hex() == \
            v["expected"], v["where"]


def test_checker_reproduces_the_helper_and_binder_vectors():
    v = G["early_secrets"][0]
    s, t = X(v["secret"]), X(v["transcript"])
    assert R.derive_secret(v["hash"], s, b"c e traffic", t).hex() == v["client_early_traffic_secret"]
    assert R.derive_secret(v["hash"], s, b"e exp master", t).hex() == v["early_exporter_master_secret"]
    v = G["handshake_secrets"][0]
    s, t = X(v["secret"]), X(v["transcript"])
    assert R.derive_secret(v["hash"], s, b"c hs traffic", t).hex() == v["client_handshake_traffic_secret"]
    assert R.derive_secret(v["hash"], s, b"s hs traffic", t).hex() == v["server_handshake_traffic_secret"]
    v = G["application_secrets"][0]
    a = R.application_stage(v["hash"], X(v["secret"]), X(v["transcript"]), 16)
    assert (a["c_ap"].hex(), a["s_ap"].hex(), a["exporter"].hex()) == \
        (v["client_application_traffic_secret_N"], v["server_application_traffic_secret_N"], v["exporter_master_secret"])
    v = G["resumption_secrets"][0]
    assert R.derive_secret(v["hash"], X(v["secret"]), b"res master", X(v["transcript"])).hex() == \
        v["resumption_master_secret"]
    v = G["psk_binder"][0]
    assert v["psk_type"] == "MBEDTLS_SSL_TLS1_3_PSK_RESUMPTION"
    assert R.psk_binder(v["hash"], X(v["psk"]), True, X(v["transcript"])).hex() == v["binder"]
    assert R.psk_binder(v["hash"], X(v["psk"]), False, X(v["transcript"])).hex() != v["binder"]


def test_checker_stage_is_the_chain_of_the_reference_vectors():
    """test_suite_ssl.data:2603-2615: 0 -> Early Secret -> Handshake Secret -> Master Secret"""
    ev = KEYS["evolve"]
    st = R.handshake_stage("sha256", None, X(ev[1]["input"]), bytes(32), 16)
    assert (st["early"].hex(), st["handshake"].hex(), st["master"].hex()) == tuple(v["expected"] for v in ev)


@pytest.mark.parametrize("hname", sorted(ALG))
def test_compression_function_of_the_checker(hname):
    blk = 64 if hname == "sha256" else 128
    for msg in (b"", b"abc", bytes(range(200))):
        pad = msg + b"\x80" + bytes((-len(msg) - 1 - blk // 8) % blk) + (8 * len(msg)).to_bytes(blk // 8, "big")
        st = R.sha2_iv(hname)
        for i in range(0, len(pad), blk):
            st = R.sha2_compress(hname, st, pad[i:i + blk])
        assert b"".join(x.to_bytes(blk // 16, "big") for x in st)[:R.HLEN[hname]] == \
            getattr(hashlib, hname)(msg).digest()


def test_library_exports_and_layouts():
    L = M.load()
    for n in NEW:
        assert hasattr(L, n), n
    assert ctypes.sizeof(_abi.CTls13HsConn) == 176 == K.HS_CONN_BYTES
    assert (_abi.CTls13HsConn.psk.offset, _abi.CTls13HsConn.shared.offset, _abi.CTls13HsConn.transcript.offset) == \
        (0, 48, 128)
    assert ctypes.sizeof(_abi.CTls13Secret) == 48 == K.SECRET_BYTES
    assert ctypes.sizeof(_abi.CTls13EarlySecrets) == 192 and ctypes.sizeof(_abi.CTls13HandshakeSecrets) == 128
    assert ctypes.sizeof(_abi.CTls13ApplicationSecrets) == 256
    assert (K.PSK_EXTERNAL, K.PSK_RESUMPTION) == (0, 1)


@pytest.mark.parametrize("hname", sorted(ALG))
def test_kernel_constants(hname):
    """the zero-salt midstates, the midstates of the "derived" secret of an
    absent PSK and Hash(""), as the batch kernels receive them"""
    f = M.load().tlsrec__tls13_ladder_consts
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_void_p]
    want = R.ladder_constants(hname)
    out = (ctypes.c_uint64 * 48)()
    assert f(ALG[hname], out) == len(want) == 32 + (8 if hname == "sha256" else 6)
    assert list(out[:len(want)]) == want
    assert f(0, out) == BAD and f(ALG[hname], None) == BAD


def test_single_shot_hash_checks_need_no_gpu():
    """a value that is no PSA hash is the reference's INTERNAL_ERROR assertion; a
    hash this library lacks and a NULL pointer are BAD_INPUT_DATA"""
    L = M.load()
    s, out = bytes(64), ctypes.create_string_buffer(256)
    n = ctypes.c_size_t(0)
    sha512 = 0x0200000b
    for alg, want in ((0, M.ERR_SSL_INTERNAL_ERROR), (0x03000009, M.ERR_SSL_INTERNAL_ERROR), (sha512, BAD)):
        for name in NEW[:4]:
            assert getattr(L, name)(alg, s, s, 32, out) == want, (name, alg)
        assert L.tlsrec_tls13_calc_finished(alg, s, s, out, ctypes.byref(n)) == want
        assert L.tlsrec_tls13_create_psk_binder(alg, s, 32, K.PSK_EXTERNAL, s, out) == want
    for name in NEW[:4]:
        assert getattr(L, name)(K.ALG_SHA_256, None, s, 32, out) == BAD
        assert getattr(L, name)(K.ALG_SHA_256, s, s, 32, None) == BAD
        assert getattr(L, name)(K.ALG_SHA_256, s, None, 32, out) == BAD
    assert L.tlsrec_tls13_calc_finished(K.ALG_SHA_256, s, s, out, None) == BAD
    assert L.tlsrec_tls13_calc_finished(K.ALG_SHA_256, None, s, out, ctypes.byref(n)) == BAD
    assert L.tlsrec_tls13_create_psk_binder(K.ALG_SHA_256, None, 32, K.PSK_EXTERNAL, s, out) == BAD
    assert L.tlsrec_tls13_create_psk_binder(K.ALG_SHA_256, s, 32, K.PSK_EXTERNAL, None, out) == BAD
    assert out.raw == bytes(256)


def test_batch_argument_errors_need_no_gpu():
    """BAD_INPUT_DATA comes before FEATURE_UNAVAILABLE: without a table nothing
    else is looked at; the two table-less batches check everything on the host"""
    L = M.load()
    p = 0x1000          # never dereferenced: every call below returns before a launch
    c = M.CIPHER_AES_128_GCM
    hs, app = L.tlsrec_tls13_keytab_derive_handshake, L.tlsrec_tls13_keytab_derive_application
    for cipher, shared in ((c, 32), (0, 32), (c, 33), (0, 33)):
        for count in (0, 4):
            assert hs(None, 0, count, cipher, 0, shared, p, p, p, p, None) == BAD
            assert app(None, 0, count, cipher, p, p, p, p, None) == BAD
    vd, ds = L.tlsrec_tls13_batch_verify_data, L.tlsrec_tls13_batch_derive_secret
    for alg in (0, 0x0200000b):
        assert vd(alg, p, p, p, 0, None) == BAD and vd(alg, p, p, p, 4, None) == BAD
        assert ds(alg, b"res master", 10, p, p, p, 0, None) == BAD
    for a in sorted(ALG.values()):
        assert vd(a, None, None, None, 0, None) == 0 and vd(a, p, p, p, 0, None) == 0
        assert vd(a, None, p, p, 4, None) == BAD and vd(a, p, None, p, 4, None) == BAD
        assert vd(a, p, p, None, 4, None) == BAD
        assert ds(a, b"res master", 10, None, None, None, 0, None) == 0
        assert ds(a, b"", 0, p, p, p, 0, None) == 0
        assert ds(a, b"x" * 13, 13, p, p, p, 0, None) == BAD          # the label comes first
        assert ds(a, None, 3, p, p, p, 0, None) == BAD
        assert ds(a, b"res master", 10, None, p, p, 4, None) == BAD
        assert ds(a, b"res master", 10, p, p, None, 4, None) == BAD
    assert ds(0, b"x" * 13, 13, p, p, p, 4, None) == BAD
