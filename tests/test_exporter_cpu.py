"""CPU-side checks of the exporter batches (include/tlsrec.h:
tlsrec_tls13_batch_exporter, tlsrec_tls12_batch_export_keying_material): the
checkers of the GPU tests pinned to the reference's own exporter vectors, to the
oracle and to OpenSSL's TLS1-PRF; the padded blocks the TLS 1.3 kernel takes as a
constant of the call; every argument error the calls decide on the host before
any launch, in the header's order; and the exports.  No test here needs a GPU."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import mbedtls_amd as M
import oracle as O
from mbedtls_amd import _abi
from mbedtls_amd import keysched as K
from mbedtls_amd import tls12 as T
from tests import exporter_ref as XR
from tests import tls12_ref as P
from tests import tls13_ref as R
from tests.prng import prng_bytes

HERE = os.path.dirname(__file__)
KEYS = json.load(open(os.path.join(HERE, "golden", "tls13_keys.json")))
HEADER = os.path.join(os.path.dirname(HERE), "include", "tlsrec.h")
X = bytes.fromhex
ALG = {"sha256": K.ALG_SHA_256, "sha384": K.ALG_SHA_384}
PRF = {"sha256": T.PRF_SHA256, "sha384": T.PRF_SHA384}
BAD, UNA = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
CALLS = ["tlsrec_tls13_batch_exporter", "tlsrec_tls12_batch_export_keying_material"]
# either side of every block boundary of the first inner message: 43 + L against 55 and 119 (SHA-256),
# 59 + L against 111 and 239 (SHA-384)
LABEL_LENS = [0, 12, 13, 52, 53, 76, 77, 249]


def test_model_reproduces_the_reference_vectors():
    vs = KEYS["exporter"]
    assert len(vs) == 3 and sorted(len(v["label"]) for v in vs) == [0, 4, 249]
    assert any(v["hash"] == "sha384" and len(v["label"]) == 249 for v in vs)
    for v in vs:
        got = XR.exporter(v["hash"], X(v["secret"]), v["label"].encode(), v["context"].encode(), v["len"])
        assert got.hex() == v["expected"], v["where"]


@pytest.mark.parametrize("hname", sorted(ALG))
def test_model_agrees_with_the_oracle(hname):
    H = R.HLEN[hname]
    for k, (ll, cl, n) in enumerate([(0, 0, 1), (4, 13, H), (19, 0, 60), (29, 1, 128), (24, 0, 32), (249, 255, 2 * H + 1),
                                     (53, 300, H - 1), (77, 56, 8160)]):
        s, lab, ctx = prng_bytes(0x3100 + k, H), prng_bytes(0x3200 + k, ll), prng_bytes(0x3300 + k, cl)
        assert XR.exporter(hname, s, lab, ctx, n) == O.tls13_exporter(ALG[hname], s, lab, ctx, n), (ll, cl, n)


@pytest.mark.parametrize("hname", sorted(PRF))
def test_tls12_model_agrees_with_openssl(hname):
    for k, (ll, ctx_len, n) in enumerate([(19, None, 60), (29, 1, 128), (24, None, 32), (0, 0, 1), (249, 255, 500),
                                          (13, 0, 48), (13, None, 48)]):
        ms, rb, lab = prng_bytes(0x3400 + k, 48), prng_bytes(0x3500 + k, 64), prng_bytes(0x3600 + k, ll)
        ctx = None if ctx_len is None else prng_bytes(0x3700 + k, ctx_len)
        seed = XR.export_seed(rb, lab, ctx)
        assert seed[:ll] == lab and seed[ll:ll + 64] == rb[32:] + rb[:32]
        assert len(seed) == ll + 64 + (0 if ctx is None else 2 + len(ctx))
        got = XR.export_keying_material(hname, ms, rb, lab, ctx, n)
        assert got == P.evp_tls1_prf(hname, ms, seed, n), (ll, ctx_len, n)
    # the empty context with use_context appends 00 00 (ssl_tls.c:8926-8929): not the same as no context
    ms, rb = prng_bytes(0x3480, 48), prng_bytes(0x3580, 64)
    assert XR.export_seed(rb, b"x", b"") == XR.export_seed(rb, b"x", None) + b"\x00\x00"
    assert XR.export_keying_material(hname, ms, rb, b"x", b"", 32) != XR.export_keying_material(hname, ms, rb, b"x", None, 32)


@pytest.mark.parametrize("hname", sorted(ALG))
def test_exporter_blocks_match_the_model(hname):
    H, blk = R.HLEN[hname], 64 if hname == "sha256" else 128
    counts = []
    for ll in LABEL_LENS:
        lab = prng_bytes(0x3800 + ll, ll)
        r, words, nblk = _abi.tls13_exporter_blocks(ALG[hname], lab)
        want, wn = XR.exporter_blocks(hname, lab)
        assert r == 0 and nblk == wn == (11 + ll + H + 1 + blk // 8 + blk - 1) // blk, ll
        assert words == want, ll
        counts.append(nblk)
        # the words are what HMAC's inner hash absorbs after the ipad block: finishing the hash by hand gives S1
        s = prng_bytes(0x3900 + ll, H)
        ip, op = R.hmac_midstates(hname, s)
        st = ip
        for b in range(nblk):
            st = R.sha2_compress(hname, st, b"".join(w.to_bytes(blk // 16, "big") for w in words[16 * b:16 * b + 16]))
        inner = b"".join(x.to_bytes(blk // 16, "big") for x in st)[:H]
        outer = inner + b"\x80" + bytes(blk - H - 1 - 8) + (8 * (blk + H)).to_bytes(8, "big")
        s1 = b"".join(x.to_bytes(blk // 16, "big") for x in R.sha2_compress(hname, op, outer))[:H]
        assert s1 == R.derive_secret(hname, s, lab, b"", hashed=False), ll
    assert counts == ([1, 1, 2, 2, 2, 2, 3, 5] if hname == "sha256" else [1, 1, 1, 1, 2, 2, 2, 3])
    f = M.load().tlsrec__tls13_exporter_blocks
    words, nblk = (ctypes.c_uint64 * 80)(), ctypes.c_uint32(7)
    assert f(0, b"x", 1, words, ctypes.byref(nblk)) == BAD
    assert f(ALG[hname], None, 1, words, ctypes.byref(nblk)) == BAD
    assert f(ALG[hname], bytes(250), 250, words, ctypes.byref(nblk)) == BAD
    assert f(ALG[hname], b"x", 1, None, ctypes.byref(nblk)) == BAD
    assert f(ALG[hname], b"x", 1, words, None) == BAD
    assert nblk.value == 7


def test_exports_bindings_and_header_agree():
    L = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rel = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for n in CALLS + ["tlsrec__tls13_exporter_blocks"]:
        assert n in rel and hasattr(L, n), n
    assert hasattr(K, "batch_exporter") and hasattr(T, "batch_export_keying_material")
    assert "batch_export_keying_material" in T.__all__
    src = open(HEADER).read()
    kinds = {ctypes.c_int: "int", ctypes.c_uint32: "uint32_t", ctypes.c_size_t: "size_t"}
    for name in CALLS:
        m = re.search(r"\bint " + name + r"\((.*?)\);", src, flags=re.S)
        assert m, name
        res, args = _abi.SIGNATURES[name]
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert res is ctypes.c_int and len(params) == len(args), name
        for p, a in zip(params, args):
            if a is ctypes.c_void_p:
                assert "*" in p, (name, p)
            else:
                assert "*" not in p and p.split()[0] == kinds[a], (name, p)


def _calls():
    """both calls behind one argument list: (alg ok?, in, label, label_len, contexts, context_len, context_stride,
    out, out_len, out_stride, count); the TLS 1.2 call with use_context set"""
    L = M.load()

    def tls13(alg_ok, inp, label, ll, ctx, cl, cs, out, ol, os_, count):
        return L.tlsrec_tls13_batch_exporter(K.ALG_SHA_256 if alg_ok else 0x0200000b, inp, label, ll, ctx, cl, cs, out,
                                             ol, os_, count, None)

    def tls12(alg_ok, inp, label, ll, ctx, cl, cs, out, ol, os_, count):
        return L.tlsrec_tls12_batch_export_keying_material(T.PRF_SHA384 if alg_ok else T.PRF_NONE, inp, label, ll, ctx,
                                                           cl, cs, 1, out, ol, os_, count, None)

    return [tls13, tls12]


@pytest.mark.parametrize("which", [0, 1])
def test_argument_errors_in_the_headers_order_need_no_gpu(which):
    """p is never dereferenced: every call returns before a launch.  Each block breaks one rule and, with it,
    every rule after it: the earlier one decides"""
    fn = _calls()[which]
    p, lab = 0x1000, b"EXPORTER-Channel-Binding"
    ok = dict(alg_ok=True, inp=p, label=lab, ll=len(lab), ctx=p, cl=8, cs=16, out=p, ol=32, os_=32, count=4)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["alg_ok"], a["inp"], a["label"], a["ll"], a["ctx"], a["cl"], a["cs"], a["out"], a["ol"], a["os_"],
                  a["count"])

    later = [dict(inp=None), dict(label=None), dict(ll=250), dict(ol=8161, os_=9000), dict(os_=31), dict(cs=7),
             dict(cl=256, cs=256)]
    # 1. the hash / the PRF, before everything else
    for kw in later + [dict(count=0), dict()]:
        assert call(alg_ok=False, **kw) == BAD
    # 2. a NULL array with count != 0
    for kw in (dict(inp=None), dict(out=None), dict(ctx=None)):
        for more in later[1:] + [dict()]:
            assert call(**dict(more, **kw)) == BAD, (kw, more)
    assert call(ctx=None, cl=0, count=0) == 0                   # contexts NULL is fine without context bytes
    assert call(inp=None, out=None, ctx=None, count=0) == 0     # ... and any array with count == 0
    # 3. label NULL with a length, 4. label_len > 249
    for more in later[3:] + [dict()]:
        assert call(label=None, **more) == BAD
        assert call(label=bytes(250), ll=250, **more) == BAD
        assert call(label=bytes(250), ll=250, count=0, **more) == BAD
    assert call(label=None, ll=0, count=0) == 0
    assert call(label=bytes(249), ll=249, count=0) == 0
    # 5. out_len > 8160, 6. out_stride < out_len, 7. a context stride shorter than the context
    assert call(ol=8161, os_=8161) == BAD and call(ol=8161, os_=8161, cl=256, cs=256) == BAD
    assert call(ol=8160, os_=8160, count=0) == 0
    assert call(os_=31) == BAD and call(os_=31, cl=256, cs=256) == BAD and call(os_=0, count=0) == BAD
    assert call(cs=7) == BAD and call(cl=256, cs=255) == BAD and call(cl=256, cs=255, count=0) == BAD
    assert call(cs=0, count=0) == 0 and call(cs=8, count=0) == 0
    # 8. FEATURE_UNAVAILABLE for a context past 255 bytes, whatever the count
    for count in (0, 4):
        assert call(cl=256, cs=256, count=count) == UNA
        assert call(cl=256, cs=0, count=count) == UNA
        assert call(cl=65535, cs=0, ol=0, os_=0, count=count) == UNA
    assert call(cl=255, cs=255, count=0) == 0
    # 9. count == 0 or out_len == 0 after the checks
    assert call(count=0) == 0 and call(ol=0, os_=0) == 0 and call(ol=0, os_=5, count=0) == 0
    assert call(ctx=None, cl=0, cs=0, ol=0) == 0


def test_tls12_call_without_use_context_ignores_the_context_arguments():
    fn = M.load().tlsrec_tls12_batch_export_keying_material
    p, lab = 0x1000, b"EXTRACTOR-dtls_srtp"
    for prf in PRF.values():
        assert fn(prf, p, lab, len(lab), None, 300, 7, 0, p, 60, 60, 0, None) == 0
        assert fn(prf, p, lab, len(lab), None, 300, 7, 1, p, 60, 60, 0, None) == BAD      # the stride, before the length
        assert fn(prf, p, lab, len(lab), None, 300, 0, 1, p, 60, 60, 0, None) == UNA
        assert fn(prf, p, lab, len(lab), None, 8, 8, 1, p, 60, 60, 4, None) == BAD        # contexts NULL, use_context
        assert fn(prf, p, lab, len(lab), None, 0, 0, 1, p, 0, 0, 4, None) == 0            # out_len == 0
    for prf in (T.PRF_NONE, 3, -1, K.ALG_SHA_256):
        assert fn(prf, None, None, 9, None, 300, 7, 1, None, 9000, 0, 4, None) == BAD


def test_python_wrappers_raise_the_code():
    p = 0x1000
    with pytest.raises(K.KeyScheduleError) as e:
        K.batch_exporter(K.ALG_SHA_384, p, b"l", p, 256, 0, p, 32, 32, 4)
    assert e.value.code == UNA
    with pytest.raises(T.KeyScheduleError) as e:
        T.batch_export_keying_material(T.PRF_SHA256, p, b"l" * 250, None, 0, 0, False, p, 32, 32, 4)
    assert e.value.code == BAD
