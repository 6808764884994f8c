"""GPU parity of the exporter batches (exporter.hip, through the C ABI):
tlsrec_tls13_batch_exporter and tlsrec_tls12_batch_export_keying_material against
the hashlib models of tests/exporter_ref.py (and, for TLS 1.3,
the oracle) -- every output byte bit-exact, and every byte around the rows
untouched, over the workgroup edges, the label, context and output lengths at
which a block count or a store path changes, strides and alignments; the
reference's own exporter vectors through the batch call; and the calls chained
after the stages that produce their inputs, on one stream with no host wait."""
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
import oracle as O  # noqa: E402
from mbedtls_amd import keysched as K  # noqa: E402
from mbedtls_amd import tls12 as T  # noqa: E402
from tests import exporter_ref as XR  # noqa: E402
from tests import tls12_hs_ref as H12  # noqa: E402
from tests import tls13_early_ref as E  # noqa: E402
from tests import tls13_ref as R  # noqa: E402
from tests.prng import prng_bytes  # noqa: E402
from tests.test_tls13_early_gpu import Out, _dev  # noqa: E402  (guarded device arrays)

HERE = os.path.dirname(__file__)
KEYS = json.load(open(os.path.join(HERE, "golden", "tls13_keys.json")))
X = bytes.fromhex
DEV = torch.device("cuda")
ALG = {"sha256": K.ALG_SHA_256, "sha384": K.ALG_SHA_384}
PRF = {"sha256": T.PRF_SHA256, "sha384": T.PRF_SHA384}
HASHES = sorted(ALG)
VERSIONS = ["tls13", "tls12"]
BAD, UNA = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
COUNTS = [1, 63, 64, 65, 130]           # one lane per connection, 64 per workgroup
LABEL_LENS = [0, 12, 13, 52, 53, 76, 77, 249]
CTX_LENS = [1, 55, 56, 63, 64, 111, 112, 119, 120, 255]
EL = {"tls13": 48, "tls12": 112}        # tlsrec_tls13_secret, tlsrec_tls12_conn
TAIL = 64                               # guard bytes past the last row
LABEL = b"EXPORTER-Channel-Binding"


def _up16(n):
    return (n + 15) & ~15


def _inputs(ver, hname, seed, count):
    """count secrets / conns; bytes of a secret past Hash.length are 0xFF: the call must not look at them"""
    raw = bytearray(prng_bytes(seed, count * EL[ver]))
    if ver == "tls13":
        hl = R.HLEN[hname]
        for i in range(count):
            raw[48 * i + hl:48 * i + 48] = b"\xff" * (48 - hl)
    return bytes(raw)


def _model(ver, hname, el, label, ctx, n):
    """one connection; ctx None = no context"""
    if ver == "tls13":
        return XR.exporter(hname, el[:R.HLEN[hname]], label, ctx or b"", n)
    return XR.export_keying_material(hname, el[:48], el[48:112], label, ctx, n)


def _call(ver, hname, inp, label, ctxs, ctx_len, ctx_stride, use, out, out_len, out_stride, count):
    if ver == "tls13":
        K.batch_exporter(ALG[hname], inp, label, ctxs, ctx_len, ctx_stride, out, out_len, out_stride, count)
    else:
        T.batch_export_keying_material(PRF[hname], inp, label, ctxs, ctx_len, ctx_stride, use, out, out_len, out_stride,
                                       count)


def _check(ver, hname, count, seed, label=LABEL, ctx_len=None, ctx_mode="each16", out_len=32, stride_mode=0,
           shifts=(0, 0, 0), raw=None, oracle=False):
    """One call against the model.  ctx_len None = no context; ctx_mode: each16 (a row per connection, the stride the
    length rounded up to 16), each (stride = length), shared (stride 0).  stride_mode: 0 out_len, 1 out_len + 3, 2 the
    next multiple of 16.  shifts: bytes past a 16-byte boundary of (secrets / conns, contexts, out).  Returns the rows."""
    raw = _inputs(ver, hname, seed, count) if raw is None else raw
    inp = _dev(raw, shifts[0])
    use = ctx_len is not None
    stride = 0
    ctxs, craw = None, b""
    if use:
        stride = {"each16": _up16(ctx_len), "each": ctx_len, "shared": 0}[ctx_mode]
        if ctx_len == 0:
            stride = 0
        craw = prng_bytes(seed + 0x5000, max(1, stride * (count - 1) + ctx_len) if stride else max(1, ctx_len))
        ctxs = _dev(craw, shifts[1])
    ostride = (out_len, out_len + 3, _up16(out_len))[stride_mode]
    total = ostride * (count - 1) + out_len
    buf = torch.full((32 + shifts[2] + total + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
    lo = 32 + shifts[2]
    view = buf[lo:lo + total]
    assert view.data_ptr() % 16 == shifts[2] % 16
    _call(ver, hname, inp, label, ctxs, ctx_len or 0, stride, use, view, out_len, ostride, count)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().tobytes()
    what = (ver, hname, count, len(label), ctx_len, ctx_mode, out_len, stride_mode, shifts)
    assert got[:lo] == b"\xa5" * lo and got[lo + total:] == b"\xa5" * TAIL, what
    rows = []
    for i in range(count):
        el = raw[EL[ver] * i:EL[ver] * (i + 1)]
        ctx = craw[stride * i:stride * i + ctx_len] if use else None
        row = got[lo + ostride * i:lo + ostride * i + out_len]
        assert row == _model(ver, hname, el, label, ctx, out_len), what + (i,)
        if oracle and ver == "tls13":
            assert row == O.tls13_exporter(ALG[hname], el[:R.HLEN[hname]], label, ctx or b"", out_len), what + (i,)
        if i + 1 < count:
            gap = got[lo + ostride * i + out_len:lo + ostride * (i + 1)]
            assert gap == b"\xa5" * (ostride - out_len), what + (i, "gap")
        rows.append(row)
    assert inp.cpu().numpy().tobytes() == raw
    if use:
        assert ctxs.cpu().numpy().tobytes() == craw
    return rows


@pytest.mark.parametrize("hname", HASHES)
@pytest.mark.parametrize("ver", VERSIONS)
def test_workgroup_edges(ver, hname):
    for count in COUNTS:
        rows = _check(ver, hname, count, 0x4000 + count, ctx_len=8, out_len=60, oracle=True)
        assert len(set(rows)) == count          # distinct secrets, distinct contexts


def _tls12_label_edges(hname):
    """the label lengths at which N + 9 or H + N + 9 (N = L + 64, the seed without a context; 9 = 0x80 and the
    length under SHA-256, 17 under SHA-384) reaches a multiple of the block, and one past it"""
    hl, bb = R.HLEN[hname], 64 if hname == "sha256" else 128
    pad = 1 + bb // 8
    lens = set()
    for extra in (0, hl):
        for m in range(bb, 64 + 249 + hl + pad + bb, bb):
            L = m - pad - 64 - extra
            lens.update(x for x in (L, L + 1) if 0 <= x <= 249)
    return sorted(lens)


@pytest.mark.parametrize("hname", HASHES)
@pytest.mark.parametrize("ver", VERSIONS)
def test_label_lengths(ver, hname):
    lens = list(LABEL_LENS)
    if ver == "tls12":
        edges = _tls12_label_edges(hname)
        assert len(edges) >= 6
        lens = sorted(set(lens) | set(edges))
    for ll in lens:
        _check(ver, hname, 65, 0x4100 + ll, label=prng_bytes(0x4180 + ll, ll), ctx_len=None, out_len=2 * R.HLEN[hname] + 1,
               oracle=ll in (0, 249))


@pytest.mark.parametrize("hname", HASHES)
@pytest.mark.parametrize("ver", VERSIONS)
def test_context_lengths(ver, hname):
    none = _check(ver, hname, 65, 0x4200, ctx_len=None)
    empty = _check(ver, hname, 65, 0x4200, ctx_len=0)
    # an empty context with use_context appends 00 00 to the TLS 1.2 seed; TLS 1.3 hashes "" either way
    assert (none == empty) == (ver == "tls13")
    for cl in CTX_LENS:
        for mode in ("each16", "each", "shared"):
            rows = _check(ver, hname, 65, 0x4200 + cl, ctx_len=cl, ctx_mode=mode, out_len=33, oracle=cl == 255)
            assert len(set(rows)) == 65


@pytest.mark.parametrize("hname", HASHES)
@pytest.mark.parametrize("ver", VERSIONS)
def test_output_lengths_and_strides(ver, hname):
    hl = R.HLEN[hname]
    for n in sorted({1, 12, hl - 1, hl, hl + 1, 2 * hl, 60, 88, 128, 8160}):
        for sm in (0, 1, 2):
            _check(ver, hname, 3 if n == 8160 else 65, 0x4300 + n, ctx_len=1, ctx_mode="shared", out_len=n, stride_mode=sm)
    _check(ver, hname, 65, 0x43FF, label=b"EXPORTER_EAP_TLS_Key_Material", ctx_len=1, ctx_mode="shared", out_len=8160,
           stride_mode=2)


@pytest.mark.parametrize("hname", HASHES)
@pytest.mark.parametrize("ver", VERSIONS)
def test_arrays_one_byte_off_alignment(ver, hname):
    for shifts in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        for n, sm in ((60, 0), (128, 2), (R.HLEN[hname] + 1, 1)):
            _check(ver, hname, 65, 0x4400 + n, ctx_len=16, out_len=n, stride_mode=sm, shifts=shifts)


@pytest.mark.parametrize("hname", HASHES)
@pytest.mark.parametrize("ver", VERSIONS)
def test_seeded_sample_of_combinations(ver, hname):
    rng = random.Random(0x4500 + 2 * HASHES.index(hname) + VERSIONS.index(ver))
    hl = R.HLEN[hname]
    for k in range(12):
        ll = rng.choice(LABEL_LENS + [19, 24, 29])
        cl = rng.choice([None, 0] + CTX_LENS)
        _check(ver, hname, rng.choice(COUNTS), 0x4500 + k, label=prng_bytes(0x4580 + k, ll), ctx_len=cl,
               ctx_mode=rng.choice(["each16", "each", "shared"]),
               out_len=rng.choice([1, 12, hl - 1, hl, hl + 1, 2 * hl, 60, 88, 128, 700]), stride_mode=rng.randrange(3),
               shifts=tuple(rng.choice([0, 0, 1, 4]) for _ in range(3)), oracle=True)


def test_reference_vectors_through_the_batch_call():
    """one label a call: each vector at count 1, and at count 65 in lane 64 behind random secrets"""
    for k, v in enumerate(KEYS["exporter"]):
        hname, hl = v["hash"], R.HLEN[v["hash"]]
        label, ctx, n = v["label"].encode(), v["context"].encode(), v["len"]
        secret = X(v["secret"]) + b"\xff" * (48 - hl)
        for count in (1, 65):
            raw = _inputs("tls13", hname, 0x4600 + k, count - 1) + secret
            cl = len(ctx) if ctx else None
            inp, out = _dev(raw), Out(count, el=_up16(n))
            K.batch_exporter(ALG[hname], inp, label, _dev(ctx) if ctx else None, len(ctx), 0, out.view, n, _up16(n), count)
            torch.cuda.synchronize()
            got = out.raw()
            assert got[_up16(n) * (count - 1):][:n].hex() == v["expected"], (v["where"], count)
            assert got[_up16(n) * (count - 1) + n:] == b"\xa5" * (_up16(n) - n)
            rows = _check("tls13", hname, count, 0, label=label, ctx_len=cl, ctx_mode="shared", out_len=n, raw=raw)
            assert cl is not None or rows[-1].hex() == v["expected"]


# ---- chains: one stream, no host wait in between -------------------------------------------
@pytest.mark.parametrize("hname", HASHES)
def test_chain_application_stage_into_the_exporter(hname):
    hl, a, count, n = R.HLEN[hname], ALG[hname], 65, 32
    cipher = M.CIPHER_AES_128_GCM if hname == "sha256" else M.CIPHER_AES_256_GCM
    mraw, traw = prng_bytes(0x4700, count * 48), prng_bytes(0x4701, count * 48)
    kt = M.KeyTable(2 * count)
    ap, ex, out = Out(2 * count), Out(count), Out(count, el=n)
    K.keytab_derive_application(kt, 0, count, cipher, _dev(mraw), _dev(traw), ap.view, ex.view)
    K.batch_exporter(a, ex.view, LABEL, None, 0, 0, out.view, n, n, count)
    torch.cuda.synchronize()
    secrets = ex.read(hl)
    assert secrets == [R.application_stage(hname, mraw[48 * i:48 * i + hl], traw[48 * i:48 * i + hl],
                                           M.KEYLEN[cipher])["exporter"] for i in range(count)]
    got = out.raw()
    for i in range(count):
        assert got[n * i:n * i + n] == XR.exporter(hname, secrets[i], LABEL, b"", n), i
    for i in (0, 31, 64):
        assert K.exporter(a, secrets[i], LABEL, b"", n) == got[n * i:n * i + n]
    kt.close()


@pytest.mark.parametrize("hname", HASHES)
def test_chain_early_stage_into_the_exporter(hname):
    hl, a, count, n = R.HLEN[hname], ALG[hname], 65, 48
    cipher = M.CIPHER_AES_128_GCM if hname == "sha256" else M.CIPHER_AES_256_GCM
    raw = prng_bytes(0x4710, count * K.PSK_CONN_BYTES)
    ctx = b"\x2a"
    kt = M.KeyTable(count)
    bd, ce, eex, out = Out(count), Out(count), Out(count), Out(count, el=n)
    K.keytab_derive_early(kt, 0, count, cipher, 32, K.PSK_RESUMPTION, _dev(raw), None, bd.view, None, ce.view, eex.view)
    K.batch_exporter(a, eex.view, b"EXPORTER_EAP_TLS_Key_Material", _dev(ctx), 1, 0, out.view, n, n, count)
    torch.cuda.synchronize()
    cb = K.PSK_CONN_BYTES
    want = [E.early_stage(hname, raw[cb * i:cb * i + 32], True, raw[cb * i + 48:cb * i + 48 + hl],
                          raw[cb * i + 96:cb * i + 96 + hl], M.KEYLEN[cipher])["e_exp"] for i in range(count)]
    assert eex.read(hl) == want
    got = out.raw()
    for i in range(count):
        assert got[n * i:n * i + n] == XR.exporter(hname, want[i], b"EXPORTER_EAP_TLS_Key_Material", ctx, n), i
    for i in (0, 64):
        assert K.exporter(a, want[i], b"EXPORTER_EAP_TLS_Key_Material", ctx, n) == got[n * i:n * i + n]
    kt.close()


@pytest.mark.parametrize("hname", HASHES)
def test_chain_master_into_the_dtls_srtp_exporter(hname):
    """master batch -> "EXTRACTOR-dtls_srtp", 60 bytes, no context (RFC 5764 4.2)"""
    count, n, label = 65, 60, b"EXTRACTOR-dtls_srtp"
    pc, cn = H12.PMS_CONN, H12.CONN
    raw = prng_bytes(0x4720, count * pc)
    conns, out = Out(count, el=cn), Out(count, el=64)
    T.tls12_batch_compute_master(PRF[hname], 48, False, _dev(raw), conns.view, count)
    T.batch_export_keying_material(PRF[hname], conns.view, label, None, 0, 0, False, out.view, n, 64, count)
    torch.cuda.synchronize()
    want = b"".join(H12.conn_out(hname, raw[pc * i:pc * i + pc], 48, False) for i in range(count))
    assert conns.raw() == want
    got = out.raw()
    for i in range(count):
        c = want[cn * i:cn * i + cn]
        assert got[64 * i:64 * i + n] == XR.export_keying_material(hname, c[:48], c[48:], label, None, n), i
        assert got[64 * i + n:64 * i + 64] == b"\xa5" * 4
    for i in (0, 33, 64):
        c = want[cn * i:cn * i + cn]
        assert T.tls12_export_keying_material(PRF[hname], c[:48], c[48:], label, None, n) == got[64 * i:64 * i + n]


@pytest.mark.parametrize("ver", VERSIONS)
def test_a_context_of_256_bytes_is_refused_and_writes_nothing(ver):
    count = 4
    for hname in HASHES:
        inp, ctxs, out = _dev(_inputs(ver, hname, 0x4800, count)), _dev(bytes(256 * count)), Out(count, el=32)
        for stride in (0, 256):
            with pytest.raises(K.KeyScheduleError) as e:
                _call(ver, hname, inp, LABEL, ctxs, 256, stride, True, out.view, 32, 32, count)
            assert e.value.code == UNA
        with pytest.raises(K.KeyScheduleError) as e:
            _call(ver, hname, inp, LABEL, ctxs, 8, 8, True, out.view, 32, 31, count)
        assert e.value.code == BAD
        _call(ver, hname, inp, LABEL, ctxs, 8, 8, True, out.view, 0, 32, count)       # out_len == 0: nothing to do
        _call(ver, hname, inp, LABEL, ctxs, 8, 8, True, out.view, 32, 32, 0)
        torch.cuda.synchronize()
        assert out.untouched()
