"""GPU parity of the DTLS cookie batch (cookie.hip through the C ABI):
tlsrec_cookie_batch_write / _check, tlsrec_dtls_check_clihlo_cookies and the
single-shot callbacks against the checker of tests/cookie_ref.py (hmac /
hashlib), every status and every output byte bit-exact -- over the id lengths
at which the inner hash takes another block, the workgroup edges, odd offsets,
every single-bit flip of a cookie, the timeout's edges, the reference's six
ClientHello vectors and synthesised ones at every bound of the parser, and one
mixed batch with canaries around every output."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import cookie as C  # noqa: E402
from tests import cookie_ref as R  # noqa: E402
from tests.prng import prng_bytes  # noqa: E402

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "dtls_cookie.json")))["cases"]
KEY, KEY2 = prng_bytes(0xC00C, 32), prng_bytes(0xC00D, 32)
NOW = 0x6703A5C7
CANARY = 0xA5
# 4 + id_len bytes are hashed: one block to 51, two from 52; 59 / 60 / 61: the message ends a byte short of, on and
# past the first block; 115 / 116: two blocks, then three; 255: five
ID_LENS = [0, 1, 6, 18, 51, 52, 59, 60, 61, 115, 116, 255]
COUNTS = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def ctx():
    c = M.CookieContext(KEY, 60)
    yield c
    c.close()


def _pack(blobs, gap=3, lead=1):
    """the blobs in one arena at odd offsets, `gap` canary bytes between them"""
    offs, pos = [], lead
    for b in blobs:
        offs.append(pos)
        pos += len(b) + gap
        pos |= 1
    a = np.full(pos + 8, CANARY, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        a[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return offs, a


def _to_dev(a):
    return torch.from_numpy(a.copy()).to(DEV)


def _ids(seed, lens):
    return [prng_bytes(seed + i, n) for i, n in enumerate(lens)]


def _cookie_batch(fn, ctx, now, ids, cookies, id_lens=None, cookie_lens=None, stream=None):
    """run batch_write / batch_check over ids[i] / cookies[i] (bytes: the space's canaries or the received cookie);
    id_lens / cookie_lens override what the items claim.  -> statuses, the cookie arena after the call, offsets, arena
    before"""
    n = len(ids)
    id_offs, ida = _pack(ids)
    ck_offs, cka = _pack(cookies)
    it = np.zeros(n, dtype=C.COOKIE_ITEM)
    for i in range(n):
        it[i] = (id_offs[i], ck_offs[i], len(ids[i]) if id_lens is None else id_lens[i],
                 len(cookies[i]) if cookie_lens is None else cookie_lens[i])
    d_id, d_ck = _to_dev(ida), _to_dev(cka)
    st = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    fn(ctx, now, it, n, d_id, d_ck, st[1:1 + n] if n else st, stream)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    assert s[0] == 0x5A5A5A5A and s[-1] == 0x5A5A5A5A
    assert d_id.cpu().numpy().tobytes() == ida.tobytes()
    return s[1:1 + n].tolist(), d_ck.cpu().numpy(), ck_offs, cka


def _write(ctx, now, ids, key=KEY, **kw):
    sts, after, offs, before = _cookie_batch(C.batch_write, ctx, now, ids, [bytes([CANARY]) * 32] * len(ids), **kw)
    out = []
    for i, cid in enumerate(ids):
        want_st, want = R.cookie_write(key, now, cid, 32)
        assert sts[i] == want_st, (i, len(cid))
        out.append(after[offs[i]:offs[i] + 32].tobytes())
        assert out[-1] == want, (i, len(cid))
        before[offs[i]:offs[i] + 32] = after[offs[i]:offs[i] + 32]
    assert after.tobytes() == before.tobytes()         # nothing but the cookies changed
    return out


# ---- write ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_write_workgroup_edges(ctx, n):
    lens = [ID_LENS[i % len(ID_LENS)] for i in range(n)]
    _write(ctx, NOW, _ids(0x100 + n, lens))


def test_write_every_id_length(ctx):
    for now in (NOW, 0, (1 << 32) - 1, (5 << 32) + 7):
        _write(ctx, now, _ids(0x200, ID_LENS))
    _write(ctx, NOW, _ids(0x300, list(range(40, 70)) + list(range(110, 125)) + [179, 180, 243, 244]))


def test_write_refusals_leave_the_space_untouched(ctx):
    ids = _ids(0x400, [6, 6, 6, 6, 6])
    spaces = [bytes([CANARY]) * 32] * 5
    sts, after, offs, before = _cookie_batch(C.batch_write, ctx, NOW, ids, spaces,
                                             id_lens=[6, 6, 256, 6, 1 << 31], cookie_lens=[31, 32, 32, 0, 64])
    assert sts == [R.BUFFER_TOO_SMALL, 0, R.BAD_INPUT_DATA, R.BUFFER_TOO_SMALL, R.BAD_INPUT_DATA]
    assert after[offs[1]:offs[1] + 32].tobytes() == R.cookie_write(KEY, NOW, ids[1], 32)[1]
    before[offs[1]:offs[1] + 32] = after[offs[1]:offs[1] + 32]
    assert after.tobytes() == before.tobytes()


# ---- check ----------------------------------------------------------------------------------
def _check(ctx, key, timeout, now, ids, cookies, **kw):
    sts, after, _, before = _cookie_batch(C.batch_check, ctx, now, ids, cookies, **kw)
    assert after.tobytes() == before.tobytes()
    want = [R.cookie_check(key, timeout, now, ck, cid)[0] for cid, ck in zip(ids, cookies)]
    assert sts == want
    return sts


def test_check_valid_over_id_lengths_and_edges(ctx):
    for n in COUNTS:
        ids = _ids(0x500 + n, [ID_LENS[(i + n) % len(ID_LENS)] for i in range(n)])
        cookies = [R.cookie_write(KEY, NOW - i % 61, cid, 32)[1] for i, cid in enumerate(ids)]
        assert _check(ctx, KEY, 60, NOW, ids, cookies) == [0] * n


def test_check_every_single_bit_flip(ctx):
    cid = prng_bytes(0x600, 6)
    good = R.cookie_write(KEY, NOW, cid, 32)[1]
    flipped = [bytes(b ^ (1 << (k % 8)) if j == k // 8 else b for j, b in enumerate(good)) for k in range(256)]
    sts = _check(ctx, KEY, 60, NOW, [cid] * 257, flipped + [good])
    assert sts == [R.INVALID_MAC] * 256 + [0]


def test_check_wrong_id_and_lengths(ctx):
    cid = prng_bytes(0x700, 18)
    good = R.cookie_write(KEY, NOW, cid, 32)[1]
    other = bytes([cid[0] ^ 0x80]) + cid[1:]
    ids = [cid, other, cid[:17], cid + b"\0", cid, cid, cid, cid]
    cookies = [good, good, good, good, b"", good[:31], good + b"\0", good]
    sts = _check(ctx, KEY, 60, NOW, ids, cookies)
    assert sts == [0, R.INVALID_MAC, R.INVALID_MAC, R.INVALID_MAC, -1, -1, -1, 0]
    # an id longer than the ABI allows
    sts, _, _, _ = _cookie_batch(C.batch_check, ctx, NOW, [cid, cid], [good, good], id_lens=[256, 18])
    assert sts == [R.BAD_INPUT_DATA, 0]


def test_check_timeout_edges():
    cid = prng_bytes(0x800, 6)
    c = M.CookieContext(KEY, 60)
    try:
        t0 = NOW
        ck = R.cookie_write(KEY, t0, cid, 32)[1]
        bad = ck[:31] + bytes([ck[31] ^ 1])
        for timeout, now, want in [(60, t0, 0), (60, t0 + 60, 0), (60, t0 + 61, -1), (60, t0 - 1, -1),
                                   (0, t0 - 1, 0), (0, t0 + (1 << 31), 0), (60, t0 + (1 << 32), -1),
                                   (0, t0 + (1 << 32), 0), (1, t0 + 1, 0), (1, t0 + 2, -1),
                                   (0xffffffff, t0 + 0xffffffff, 0), (0xffffffff, t0 + (1 << 32), -1)]:
            c.set_timeout(timeout)                       # set_timeout takes effect
            assert _check(c, KEY, timeout, now, [cid, cid], [ck, bad]) == [want, R.INVALID_MAC], (timeout, now)
    finally:
        c.close()


# ---- ClientHello ----------------------------------------------------------------------------
def _hello(seed, sid_len=0, cookie=b"", tail=b"\x00\x02\xc0\x2b\x01\x00", typ=22, epoch=b"\0\0", frag=b"\0\0\0"):
    """a DTLS 1.2 ClientHello datagram with its record sequence number and message_seq taken from seed"""
    sid = prng_bytes(seed + 1, sid_len)
    body = b"\xfe\xfd" + prng_bytes(seed + 2, 32) + bytes([sid_len]) + sid + bytes([len(cookie)]) + cookie + tail
    seq = prng_bytes(seed + 3, 6)
    mseq = prng_bytes(seed + 4, 2)
    hs = b"\x01" + len(body).to_bytes(3, "big") + mseq + frag + len(body).to_bytes(3, "big") + body
    return bytes([typ]) + b"\xfe\xfd" + epoch + seq + len(hs).to_bytes(2, "big") + hs


def _clihlo(ctx, key, timeout, now, items, id_lens=None):
    """items: (datagram, cli_id, out_cap).  Runs the batch, checks every status, olen and output byte and every
    canary against the checker; returns the statuses and outputs."""
    n = len(items)
    offs, arena = _pack([d for d, _, _ in items])
    id_offs, ida = _pack([c for _, c, _ in items])
    out_offs, outa = _pack([bytes([CANARY]) * cap for _, _, cap in items], gap=5)
    h = np.zeros(n, dtype=C.CLIHLO)
    for i, (d, cid, cap) in enumerate(items):
        h[i] = (offs[i], id_offs[i], out_offs[i], len(d), len(cid) if id_lens is None else id_lens[i], cap, 0)
    d_in, d_id, d_out = _to_dev(arena), _to_dev(ida), _to_dev(outa)
    res = torch.full((8 * (n + 2),), 0x5A, dtype=torch.uint8, device=DEV)
    C.check_clihlo(ctx, now, h, n, d_in, d_id, d_out, res[8:8 + 8 * n])
    torch.cuda.synchronize()
    raw = res.cpu().numpy()
    assert raw[:8].tobytes() == b"\x5a" * 8 and raw[-8:].tobytes() == b"\x5a" * 8
    got = np.frombuffer(raw[8:8 + 8 * n].tobytes(), dtype=C.CLIHLO_RES)
    assert d_in.cpu().numpy().tobytes() == arena.tobytes() and d_id.cpu().numpy().tobytes() == ida.tobytes()
    after = d_out.cpu().numpy()
    sts, outs = [], []
    for i, (d, cid, cap) in enumerate(items):
        cid_ref = cid if id_lens is None or id_lens[i] == len(cid) else None
        want_st, want = R.check_clihlo(key, timeout, now, cid_ref, d, cap)
        assert (int(got["status"][i]), int(got["olen"][i])) == (want_st, len(want)), (i, len(d), cap)
        outa[out_offs[i]:out_offs[i] + len(want)] = np.frombuffer(want, dtype=np.uint8)
        sts.append(want_st)
        outs.append(after[out_offs[i]:out_offs[i] + len(want)].tobytes())
    # the HelloVerifyRequests byte for byte; every other byte of the arena (the canaries, the spaces of the items
    # that passed, failed to decode or had no room) as it was
    assert after.tobytes() == outa.tobytes()
    return sts, outs


CLI = b"\xc0\xa8\x01\x07\xd4\x31"


def test_clihlo_reference_vectors(ctx):
    items = []
    for c in CASES:
        for cap in (0, 27, 28, 59, 60, 61, 16384):
            items.append((bytes.fromhex(c["datagram"]), CLI, cap))
    sts, _ = _clihlo(ctx, KEY, 60, NOW, items)
    k = 0
    for c in CASES:
        for cap in (0, 27, 28, 59, 60, 61, 16384):
            if c["ret"] == R.DECODE_ERROR:
                assert sts[k] == R.DECODE_ERROR, c["name"]
            elif 28 <= cap < 60:
                assert sts[k] == c["ret"] == R.INTERNAL_ERROR          # the reference's recorded result
            else:
                assert sts[k] == (R.BUFFER_TOO_SMALL if cap < 28 else R.HELLO_VERIFY_REQUIRED)
            k += 1


def _synth(now):
    """hellos at every bound of the parser: (datagram, cli_id, out_cap)"""
    good = R.cookie_write(KEY, now, CLI, 32)[1]
    bad = good[:13] + bytes([good[13] ^ 0x10]) + good[14:]
    items, seed = [], 0x900
    for sid_len in (0, 32, 255):
        for ck in (b"", good[:31], good, bad, prng_bytes(seed, 255)):
            seed += 8
            d = _hello(seed, sid_len, ck)
            full = 61 + sid_len + len(ck)              # the datagram may end right after the cookie
            for ln in {len(d), full, full - 1, 61 + sid_len, 60 + sid_len, 61, 60}:
                if 0 < ln <= len(d):
                    items.append((d[:ln], CLI, 60))
    for kw in (dict(typ=23), dict(epoch=b"\0\1"), dict(epoch=b"\1\0"), dict(frag=b"\1\0\0"), dict(frag=b"\0\1\0"),
               dict(frag=b"\0\0\1")):
        seed += 8
        items.append((_hello(seed, 0, good, **kw), CLI, 60))
        items.append((_hello(seed, 0, b"", **kw), CLI, 60))
    for cap in (0, 27, 28, 59, 60, 61):
        for ck in (good, bad, b""):
            seed += 8
            items.append((_hello(seed, 32, ck), CLI, cap))
    return items


def test_clihlo_synthesised_bounds(ctx):
    items = _synth(NOW)
    sts, _ = _clihlo(ctx, KEY, 60, NOW, items)
    assert {0, R.DECODE_ERROR, R.BUFFER_TOO_SMALL, R.INTERNAL_ERROR, R.HELLO_VERIFY_REQUIRED} == set(sts)
    # expired and future cookies take the HelloVerifyRequest path; without a timeout they pass
    good = R.cookie_write(KEY, NOW, CLI, 32)[1]
    d = _hello(0xA00, 0, good)
    assert _clihlo(ctx, KEY, 60, NOW + 61, [(d, CLI, 60)])[0] == [R.HELLO_VERIFY_REQUIRED]
    assert _clihlo(ctx, KEY, 60, NOW - 1, [(d, CLI, 60)])[0] == [R.HELLO_VERIFY_REQUIRED]
    assert _clihlo(ctx, KEY, 60, NOW + 60, [(d, CLI, 60)])[0] == [0]


def test_clihlo_long_ids_and_bad_id_len(ctx):
    items = []
    for k, n in enumerate(ID_LENS):
        cid = prng_bytes(0xB00 + k, n)
        items.append((_hello(0xB40 + 8 * k, 0, b""), cid, 60))
        items.append((_hello(0xB44 + 8 * k, 32, R.cookie_write(KEY, NOW - 3, cid, 32)[1]), cid, 60))
    sts, _ = _clihlo(ctx, KEY, 60, NOW, items)
    assert sts == [R.HELLO_VERIFY_REQUIRED, 0] * len(ID_LENS)
    d = _hello(0xBF0, 0, R.cookie_write(KEY, NOW, CLI, 32)[1])
    sts, _ = _clihlo(ctx, KEY, 60, NOW, [(d, CLI, 60), (d, CLI, 27), (d[:60], CLI, 60)], id_lens=[256, 256, 256])
    assert sts == [R.INTERNAL_ERROR, R.BUFFER_TOO_SMALL, R.DECODE_ERROR]


def test_clihlo_round_trip(ctx):
    other = b"\xc0\xa8\x01\x07\xd4\x32"
    first = _hello(0xC00, 32, b"")
    sts, outs = _clihlo(ctx, KEY, 60, NOW, [(first, CLI, 60)])
    assert sts == [R.HELLO_VERIFY_REQUIRED]
    hvr = outs[0]
    assert hvr[:11] == first[:11] and hvr[13] == 3 and hvr[17:19] == first[17:19] and hvr[27] == 32
    second = _hello(0xC00, 32, hvr[28:60])
    sts, _ = _clihlo(ctx, KEY, 60, NOW + 2, [(second, CLI, 60), (second, other, 60)])
    assert sts == [0, R.HELLO_VERIFY_REQUIRED]


def test_clihlo_mixed_batch_of_193(ctx):
    pool = _synth(NOW)
    by = {}
    for it in pool:
        by.setdefault(R.check_clihlo(KEY, 60, NOW, it[1], it[0], it[2])[0], []).append(it)
    assert len(by) == 5
    kinds = sorted(by)
    items = [by[kinds[i % 5]][(i // 5) % len(by[kinds[i % 5]])] for i in range(193)]
    # give the items that write nothing a space to leave untouched, of a size of their own
    items = [(d, c, cap if R.check_clihlo(KEY, 60, NOW, c, d, cap)[0] not in (0, R.DECODE_ERROR) else 60 + i % 7)
             for i, (d, c, cap) in enumerate(items)]
    sts, _ = _clihlo(ctx, KEY, 60, NOW, items)
    assert len(sts) == 193 and set(sts) == set(kinds)


# ---- contexts -------------------------------------------------------------------------------
def test_two_keys_give_different_cookies(ctx):
    ids = _ids(0xD00, [6, 18, 60])
    a = _write(ctx, NOW, ids)
    c2 = M.CookieContext(KEY2, 60)
    try:
        b = _write(c2, NOW, ids, key=KEY2)
        assert all(x[:4] == y[:4] and x[4:] != y[4:] for x, y in zip(a, b))
        assert _check(c2, KEY2, 60, NOW, ids, b) == [0] * 3
        assert _check(c2, KEY2, 60, NOW, ids, a) == [R.INVALID_MAC] * 3
    finally:
        c2.close()


def test_random_key_contexts():
    a, b = M.CookieContext(None), M.CookieContext(None, 0)
    try:
        ids = _ids(0xE00, [6, 52])
        outs = []
        for c in (a, b):
            sts, after, offs, _ = _cookie_batch(C.batch_write, c, NOW, ids, [bytes(32)] * 2)
            assert sts == [0, 0]
            outs.append([after[o:o + 32].tobytes() for o in offs])
        assert all(x[:4] == NOW.to_bytes(4, "big") for x in outs[0] + outs[1])
        assert outs[0][0][4:] != outs[1][0][4:] and outs[0][1][4:] != outs[1][1][4:]
        for c, mine, theirs in ((a, outs[0], outs[1]), (b, outs[1], outs[0])):
            assert _cookie_batch(C.batch_check, c, NOW + 5, ids, mine)[0] == [0, 0]
            assert _cookie_batch(C.batch_check, c, NOW + 5, ids, theirs)[0] == [R.INVALID_MAC] * 2
    finally:
        a.close()
        b.close()


def test_single_shot_callbacks(ctx):
    import time
    for n in (0, 6, 51, 52, 255):
        cid = prng_bytes(0xF00 + n, n)
        t0 = int(time.time())
        st, ck, moved = ctx.write(cid, 40)
        t1 = int(time.time())
        assert (st, moved, len(ck)) == (0, 32, 32)
        stamp = int.from_bytes(ck[:4], "big")
        assert t0 <= stamp <= t1
        assert ck == R.cookie_write(KEY, stamp, cid, 32)[1]
        # the batch of one, stamped alike
        assert _write(ctx, stamp, [cid]) == [ck]
        assert ctx.check(ck, cid) == 0
        assert ctx.check(ck[:31] + bytes([ck[31] ^ 1]), cid) == R.INVALID_MAC
        assert ctx.check(ck, cid + b"x") == (R.INVALID_MAC if n < 255 else R.BAD_INPUT_DATA)
        for bad in (b"", ck[:31], ck + b"\0"):
            assert ctx.check(bad, cid) == -1
    old = R.cookie_write(KEY, int(time.time()) - 3600, b"peer", 32)[1]
    assert ctx.check(old, b"peer") == -1
    assert ctx.write(b"peer", 31) == (R.BUFFER_TOO_SMALL, b"", 0)
    assert ctx.write(b"x" * 256, 32) == (R.BAD_INPUT_DATA, b"", 0)


def test_non_default_stream_and_empty_batch(ctx):
    s = torch.cuda.Stream()
    ids = _ids(0x1000, [6] * 65)
    with torch.cuda.stream(s):
        sts, after, offs, _ = _cookie_batch(C.batch_write, ctx, NOW, ids, [bytes(32)] * 65, stream=s)
    assert sts == [0] * 65
    cookies = [after[o:o + 32].tobytes() for o in offs]
    assert cookies == [R.cookie_write(KEY, NOW, cid, 32)[1] for cid in ids]
    assert _cookie_batch(C.batch_check, ctx, NOW, ids, cookies, stream=s)[0] == [0] * 65
    # n = 0: nothing runs, nothing is looked at
    L = M.load()
    assert L.tlsrec_cookie_batch_write(ctx.handle, NOW, None, 0, None, None, None, None) == 0
    assert L.tlsrec_cookie_batch_check(ctx.handle, NOW, None, 0, None, None, None, None) == 0
    assert L.tlsrec_dtls_check_clihlo_cookies(ctx.handle, NOW, None, 0, None, None, None, None, None) == 0
