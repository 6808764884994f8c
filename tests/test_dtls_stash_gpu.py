"""DTLS receive framing under every dispatch of tlsrec_dtls_decrypt, against
the oracle (oracle/dtls.c), each test asserting the path it was built for from
the dispatchers' launch log (the test-hooks build):

  * dtls_frame_kernel<16> (the 96 KiB LDS stash of the first 16 records of a
    connection, 4 < ceil(datagrams / connections) <= 16), <4> and <0>, with
    TLSREC_DTLS_STASH=0 and the count / scan / emit kernels as second paths,
    all over the same per-connection content;
  * the stash's epoch / 48-bit sequence number decode with every byte of the
    window's top set;
  * descriptors past max_records are never written, by any DTLS or stream
    receive framing (canaries behind the caller's capacity).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402
from mbedtls_amd import dtls as D  # noqa: E402
from mbedtls_amd import stream as S  # noqa: E402
import oracle as O  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests.batchlib import launch_log  # noqa: E402,F401  (fixture)
from tests.prng import prng_bytes  # noqa: E402
from tests.test_stream_gpu import FRAMINGS as STREAM_FRAMINGS, FRAMING_IDS as STREAM_FRAMING_IDS  # noqa: E402
from tests.test_stream_gpu import _framing as _stream_framing  # noqa: E402

DEV = torch.device("cuda")


def ctr(epoch, seq):
    return epoch.to_bytes(2, "big") + (seq % (1 << 48)).to_bytes(6, "big")


def _per(conns):
    """ceil(datagrams / connections): what tlsrec_dtls_decrypt picks the stash depth from"""
    nd = sum(len(c[2]) for c in conns)
    return (nd + len(conns) - 1) // len(conns)


def _expected_s(per, stash, fused):
    if fused == "0":
        return -1
    return 0 if (stash == "0" or per > 16) else (16 if per > 4 else 4)


# (TLSREC_DTLS_STASH, TLSREC_GROUPED, TLSREC_RX_FUSED)
LEGS = [(None, "1", "1"), (None, "0", "1"), ("0", "1", "1"), ("0", "0", "1"), (None, "1", "0")]
LEG_IDS = ["stash-grouped", "stash-bucket", "nostash-grouped", "nostash-bucket", "three-kernels"]


def _leg(monkeypatch, leg):
    stash, grouped, fused = leg
    if stash is None:
        monkeypatch.delenv("TLSREC_DTLS_STASH", raising=False)
    else:
        monkeypatch.setenv("TLSREC_DTLS_STASH", stash)
    monkeypatch.setenv("TLSREC_GROUPED", grouped)
    monkeypatch.setenv("TLSREC_RX_FUSED", fused)


# ---- the record mix -------------------------------------------------------------
# slot: (cipher, key, iv, cid); slots 1..6 carry CIDs of 1..6 bytes (the cid_len
# byte of the stash word), slot 7 is CCM_8, slot 8 is loaded as TLS 1.3 (unusable)
def _mix_slots():
    ciphers = [M.CIPHER_AES_128_GCM, M.CIPHER_CHACHA20_POLY1305, M.CIPHER_AES_256_GCM, M.CIPHER_AES_128_GCM,
               M.CIPHER_AES_192_GCM, M.CIPHER_CHACHA20_POLY1305, M.CIPHER_AES_256_GCM, M.CIPHER_AES_256_CCM_8,
               M.CIPHER_AES_128_GCM]
    cids = [0, 1, 2, 3, 4, 5, 6, 0, 0]
    out = []
    for i, (c, n) in enumerate(zip(ciphers, cids)):
        b = prng_bytes(8800 + i, 48)
        out.append((c, b[:M.KEYLEN[c]], b[32:48], prng_bytes(8900 + i, n) if n else b""))
    return out


BAD_SLOT = 8
COUNTS = [0, 1, 15, 16, 17, 5, 9, 12, 7, 3, 16, 11]      # records of connection i: COUNTS[i % 12]
NBASE = 324                                              # two tiles of 256 lanes
LONG_AT, BAD_AT = 100, 131                               # the 40-record connection, the TLS 1.3 slot's


@functools.lru_cache(maxsize=None)
def _mix(scale):
    """(slots, conns): NBASE connections whose datagrams per connection average
    in (4, 16]; scale 4 appends one-datagram connections until the mean is at
    most 4, scale 0 appends long connections until it is above 16 -- the base
    connections' content is the same under each."""
    slots = _mix_slots()
    ot = []
    for c, k, iv, cid in slots:
        t = O.Transform(O.TLS1_2, c, k, k, iv, iv)
        t.set_cid(cid, cid)
        ot.append(t)

    @functools.lru_cache(maxsize=None)
    def rec(slot, seq, epoch=1, n=None):
        n = 20 + (seq * 5 + slot) % 23 if n is None else n
        st, w, _, _ = O.dtls_encrypt(ot[slot], prng_bytes(seq + 131 * slot, n), 23, ctr(epoch, seq), 16384)
        assert st == 0
        return w

    def flip(w, at):
        b = bytearray(w)
        b[at] ^= 0x10
        return bytes(b)

    def plain(slot, count, pack):
        """`count` records, sequence numbers 1.., `pack` of them per datagram"""
        grams, k = [], 1
        while k <= count:
            m = min(pack, count - k + 1)
            grams.append(b"".join(rec(slot, k + j) for j in range(m)))
            k += m
        return grams

    r = [None] + [rec(0, k) for k in range(1, 10)]
    special = {
        # a bad MAC with a record after it in the datagram (dropped with it), then more records
        20: (0, {"in_epoch": 1}, [r[1], flip(r[2], 30) + r[3], r[4], r[5], r[6]]),
        # a replay
        21: (0, {"in_epoch": 1}, [r[1], r[2], r[1], r[3], r[4], r[2] + r[5]]),
        # a trailing byte
        22: (0, {"in_epoch": 1}, [r[1] + b"\x17", r[2], r[3], r[4], r[5]]),
        # the next and the previous epoch
        23: (0, {"in_epoch": 1}, [r[1], rec(0, 2, epoch=2), rec(0, 3, epoch=0), r[4], r[5], r[6]]),
        # an empty datagram
        24: (0, {"in_epoch": 1}, [r[1], b"", r[2], r[3], r[4]]),
        # truncated headers
        25: (0, {"in_epoch": 1}, [r[1][:9], r[2], r[3][:-1], r[4], r[5] + r[6][:12]]),
        # badmac_limit reached: fatal, the rest not reached
        26: (0, {"in_epoch": 1, "badmac_limit": 2}, [r[1], flip(r[2], 30), r[3], flip(r[4], 30), r[5], r[6]]),
        # a window carried in
        27: (0, {"in_epoch": 1, "window_top": 7, "window": 0b1010011}, [r[7], r[6], r[5], r[4], r[3], r[2], r[9]]),
        # the re-walk (more records than any stash holds) between stashed lanes
        LONG_AT: (0, {"in_epoch": 1}, plain(0, 40, 1)),
        # an unusable slot: BAD_INPUT_DATA, no records
        BAD_AT: (BAD_SLOT, {"in_epoch": 1}, [r[1], r[2], r[3], r[4], r[5]]),
    }
    conns, seen = [], set()
    for i in range(NBASE):
        if i in special:
            conns.append(special[i])
            continue
        slot = (5 * i + i // 12) % 8
        count, pack = COUNTS[i % 12], (1, 2, 3)[(i // 12) % 3]     # one record per datagram, or 2 / 3 packed
        seen.add((count, pack))
        conns.append((slot, {"in_epoch": 1, "cid_len": len(slots[slot][3])}, plain(slot, count, pack)))
    assert 4 < _per(conns) <= 16
    assert {(n, k) for n in (0, 1, 15, 16, 17) for k in (1, 2, 3)} <= seen
    assert {c[0] for c in conns} == set(range(9))
    if scale == 4:
        k = 0
        while _per(conns) > 4:
            conns.append((k % 8, {"in_epoch": 1, "cid_len": len(slots[k % 8][3])}, plain(k % 8, 1, 1)))
            k += 1
    elif scale == 0:
        while _per(conns) <= 16:
            conns.append((0, {"in_epoch": 1}, plain(0, 700, 1)))
    return slots, conns


def _run_mix(scale, leg, monkeypatch, launch_log):
    _leg(monkeypatch, leg)
    slots, conns = _mix(scale)
    per = _per(conns)
    assert {16: 4 < per <= 16, 4: per <= 4, 0: per > 16}[scale]
    tab = B.Table(slots, tls_of={BAD_SLOT: M.VERSION_TLS1_3})
    launch_log.reset()
    got = tab.decrypt(conns)
    frames = launch_log(_abi.LOG_DTLS_RX_FRAME)
    assert frames == [(_abi.LOG_DTLS_RX_FRAME, _expected_s(per, leg[0], leg[2]), 0, 0, 0)], frames
    assert [e[1] for e in launch_log(_abi.LOG_BUCKET)] == [1 if leg[1] == "0" else 0]
    B.check_vs_oracle(tab, conns, got, skip={BAD_AT})
    cres = got[4]
    assert int(cres[BAD_AT]["status"]) == M.ERR_SSL_BAD_INPUT_DATA and int(cres[BAD_AT]["nrec"]) == 0
    assert int(cres[LONG_AT]["nrec"]) == 40 and int(cres[LONG_AT]["naccepted"]) == 40
    tab.close()


@pytest.mark.parametrize("leg", LEGS, ids=LEG_IDS)
def test_stash_16_mixed_tile(leg, monkeypatch, launch_log):
    """324 connections (two tiles: the look-back carries), 0 / 1 / 15 / 16 / 17
    and other record counts, one record per datagram and 2-3 packed, a
    40-record connection (the re-walk) between stashed lanes, a bad MAC with
    records after it, a replay, a trailing byte, both neighbouring epochs, an
    empty datagram, truncated headers, badmac_limit reached, CIDs of 1-6
    bytes, a CCM_8 slot and a TLS 1.3 slot (BAD_INPUT_DATA, its neighbours
    right): dtls_frame_kernel<16> by default."""
    _run_mix(16, leg, monkeypatch, launch_log)


@pytest.mark.parametrize("leg", LEGS, ids=LEG_IDS)
def test_same_mix_stash_4(leg, monkeypatch, launch_log):
    """The same connections followed by one-datagram ones: dtls_frame_kernel<4>,
    where most of the mix re-walks."""
    _run_mix(4, leg, monkeypatch, launch_log)


@pytest.mark.parametrize("leg", LEGS, ids=LEG_IDS)
def test_same_mix_no_stash(leg, monkeypatch, launch_log):
    """The same connections followed by 700-datagram ones (mean above 16):
    dtls_frame_kernel<0>."""
    _run_mix(0, leg, monkeypatch, launch_log)


# ---- high sequence numbers ------------------------------------------------------
TOP = 0xA1B2C3D4E5F6
WINDOW = 0xF0F000000F0F5A5B            # bit 0: TOP itself was seen
EPOCH = 0x1234


def _high_seqs():
    """Sequence numbers around a window top with all six bytes set: TOP +- 2^(8b)
    for every byte b, the window's edges, and -- TOP's bytes ascend from the
    high one down -- for every byte k the number with byte k one above TOP's
    and the bytes below it zero: fresh, but older than the window as soon as
    byte k is exchanged with any lower byte.  Stale ones first, then ascending
    (each fresh when it arrives)."""
    below, above = [TOP, TOP - 63, TOP - 64, TOP - 1, TOP - 2, TOP - 4], [TOP + 1, TOP + 65]
    for b in range(6):
        if TOP - (1 << 8 * b) >= 0:
            below.append(TOP - (1 << 8 * b))
        if TOP + (1 << 8 * b) < 1 << 48:
            above.append(TOP + (1 << 8 * b))
    for k in range(1, 6):
        above.append(((TOP >> 8 * k) + 1) << 8 * k)
    above = sorted(set(above))
    assert all(TOP < s < 1 << 48 for s in above) and len(above) >= 12
    return below, above


@pytest.mark.parametrize("stash", [4, 16])
def test_high_sequence_numbers(stash, monkeypatch, launch_log):
    """Every connection arrives with window_top = 0xA1B2C3D4E5F6 and a
    non-trivial window and holds at most `stash` records, so each descriptor's
    slot / NO_SLOT comes from the stash's rebuilt epoch and sequence number; a
    record of an epoch that differs from in_epoch in the high byte only (and
    one with the bytes exchanged) among them."""
    _leg(monkeypatch, (None, "1", "1"))
    key, iv = prng_bytes(61, 16), prng_bytes(62, 16)
    tab = B.Table([(M.CIPHER_AES_128_GCM, key, iv, b"")])
    t = tab.ot[0]

    def rec(seq, epoch=EPOCH):
        st, w, _, _ = O.dtls_encrypt(t, prng_bytes(seq & 0xFFFFFF, 33), 23, ctr(epoch, seq), 16384)
        assert st == 0
        return w

    below, above = _high_seqs()
    per = 4 if stash == 4 else 9
    grams = [rec(s) for s in below] + [rec(TOP + 1, epoch=0x1334), rec(TOP + 1, epoch=0x3412)] + \
        [rec(s) for s in above]
    state = {"in_epoch": EPOCH, "window_top": TOP, "window": WINDOW}
    conns = [(0, dict(state), grams[k:k + per]) for k in range(0, len(grams), per)]
    # ... and one connection per fresh number alone in front of stale ones (its window moves last)
    conns += [(0, dict(state), [rec(TOP - 64), rec(TOP), rec(s)]) for s in above]
    while (_per(conns) > 4) != (stash == 16):       # steer the mean: pad with full / with one-record connections
        conns.append((0, dict(state), grams[:per] if stash == 16 else [rec(TOP + 2)]))
    assert max(len(c[2]) for c in conns) <= stash
    launch_log.reset()
    got = tab.decrypt(conns)
    assert launch_log(_abi.LOG_DTLS_RX_FRAME) == [(_abi.LOG_DTLS_RX_FRAME, stash, 0, 0, 0)]
    B.check_vs_oracle(tab, conns, got)
    # the oracle's word on the interesting ones, spelled out: every number above the top is accepted
    cres, disp = got[4], got[3]
    for i in range(len(conns)):
        if len(conns[i][2]) == 3 and conns[i][2][0] == rec(TOP - 64):
            f = int(cres[i]["first"])
            assert [int(x) for x in disp[f:f + 3]] == [M.ERR_SSL_UNEXPECTED_RECORD, M.ERR_SSL_UNEXPECTED_RECORD, 0], i
    tab.close()


# ---- descriptors past max_records ------------------------------------------------
CANARY = 0xA5


def _canaried(T):
    recs = torch.full(((T + 8) * 40,), CANARY, dtype=torch.uint8, device=DEV)
    res = torch.full(((T + 8) * 16,), CANARY, dtype=torch.uint8, device=DEV)
    return recs, res


def _untouched(t, item, first):
    return bool((t.cpu().numpy()[first * item:] == CANARY).all())


# (ceil(datagrams / connections), TLSREC_RX_FUSED, the S the log must show)
DTLS_GUARD = [(3, "1", 4), (6, "1", 16), (17, "1", 0), (6, "0", -1)]


@pytest.mark.parametrize("per,fused,want_s", DTLS_GUARD, ids=["S4", "S16", "S0", "three-kernels"])
def test_dtls_max_records_guard(per, fused, want_s, monkeypatch, launch_log):
    """260 connections (two tiles) of `per` one-record datagrams, T records in
    all; recs / res hold T + 8 entries of 0xA5.  max_records below T:
    BUFFER_TOO_SMALL, no entry from max_records on written, nothing decrypted;
    max_records = T: success, the 8 entries behind untouched."""
    _leg(monkeypatch, (None, "1", fused))
    tab = B.Table([(M.CIPHER_AES_128_GCM, prng_bytes(71, 16), prng_bytes(72, 16), b""),
                   (M.CIPHER_CHACHA20_POLY1305, prng_bytes(73, 32), prng_bytes(74, 16), b"")])
    grams = [[O.dtls_encrypt(tab.ot[s], prng_bytes(700 + k, 24), 23, ctr(1, k + 1), 16384)[1] for k in range(per)]
             for s in range(2)]
    conns = [(i % 2, {"in_epoch": 1}, grams[i % 2]) for i in range(260)]
    d, dg, ndg, a, offs, _ = tab.layout_in(conns)
    T = 260 * per
    for max_records in (T - 1, T - 7, 1):
        ta = torch.from_numpy(a).to(DEV)
        recs, res = _canaried(T)
        disp = torch.full((T + 8,), -1, dtype=torch.int32, device=DEV)
        cres = torch.zeros(len(conns) * 48, dtype=torch.uint8, device=DEV)
        launch_log.reset()
        with pytest.raises(S.StreamError) as e:
            D.decrypt(tab.kt, d, len(conns), dg, ndg, ta, recs, res, disp, max_records, cres)
        torch.cuda.synchronize()
        assert e.value.code == M.ERR_SSL_BUFFER_TOO_SMALL
        assert launch_log(_abi.LOG_DTLS_RX_FRAME) == [(_abi.LOG_DTLS_RX_FRAME, want_s, 0, 0, 0)]
        assert _untouched(recs, 40, max_records), max_records
        assert _untouched(res, 16, max_records), max_records
        assert (disp.cpu().numpy() == -1).all()
        assert (ta.cpu().numpy() == a).all(), "decrypted although the call failed"
    ta = torch.from_numpy(a).to(DEV)
    recs, res = _canaried(T)
    disp = torch.full((T + 8,), -1, dtype=torch.int32, device=DEV)
    cres = torch.zeros(len(conns) * 48, dtype=torch.uint8, device=DEV)
    assert D.decrypt(tab.kt, d, len(conns), dg, ndg, ta, recs, res, disp, T, cres) == T
    torch.cuda.synchronize()
    assert _untouched(recs, 40, T) and _untouched(res, 16, T) and (disp.cpu().numpy()[T:] == -1).all()
    B.check_vs_oracle(tab, conns, (ta.cpu().numpy(), recs.cpu().numpy()[:T * 40].view(M.BATCH_REC),
                                   res.cpu().numpy()[:T * 16].view(M.BATCH_RES), disp.cpu().numpy(),
                                   cres.cpu().numpy().view(D.DTLS_IN_RES), offs))
    tab.close()


@pytest.mark.parametrize("fr", STREAM_FRAMINGS, ids=STREAM_FRAMING_IDS)
def test_stream_max_records_guard(fr, monkeypatch, launch_log):
    """The same for tlsrec_stream_decrypt under each of its framings: 300
    connections (more than one tile of every one-pass shape) of 3 records."""
    _stream_framing(monkeypatch, fr)
    gw, grouped, fused, rg = fr
    slots = [(M.CIPHER_AES_128_GCM, M.VERSION_TLS1_3, prng_bytes(81, 16), prng_bytes(82, 12), 0),
             (M.CIPHER_CHACHA20_POLY1305, M.VERSION_TLS1_2, prng_bytes(83, 32), prng_bytes(84, 12), 0),
             (M.CIPHER_AES_256_GCM, M.VERSION_TLS1_2, prng_bytes(85, 32), prng_bytes(86, 12), 0)]
    c = B.Conns(slots)
    wires = []
    for s in range(3):
        pt = prng_bytes(870 + s, 3 * 40 - s)
        st, w, nrec, _ = O.stream_encrypt(c.ot[s], pt, 23, (5 + s).to_bytes(8, "big"), 40)
        assert st == 0 and nrec == 3
        wires.append(w)
    conns = [(i % 3, wires[i % 3], 5 + i % 3, 0) for i in range(300)]
    d, a, offs, _ = c.layout_in(conns)
    T = 900
    want_log = [(_abi.LOG_STREAM_RX_FRAME, int(fused == "1" and gw == "1"), int(rg) if gw == "1" else 1, 0, 0)]
    for max_records in (T - 1, T - 7, 1):
        ta = torch.from_numpy(a).to(DEV)
        recs, res = _canaried(T)
        sres = torch.zeros(len(conns) * 32, dtype=torch.uint8, device=DEV)
        launch_log.reset()
        with pytest.raises(S.StreamError) as e:
            S.decrypt(c.kt, d, len(conns), ta, recs, res, max_records, sres)
        torch.cuda.synchronize()
        assert e.value.code == M.ERR_SSL_BUFFER_TOO_SMALL
        assert launch_log(_abi.LOG_STREAM_RX_FRAME) == want_log
        assert _untouched(recs, 40, max_records), max_records
        assert _untouched(res, 16, max_records), max_records
        assert (ta.cpu().numpy() == a).all(), "decrypted although the call failed"
    ta = torch.from_numpy(a).to(DEV)
    recs, res = _canaried(T)
    sres = torch.zeros(len(conns) * 32, dtype=torch.uint8, device=DEV)
    launch_log.reset()
    assert S.decrypt(c.kt, d, len(conns), ta, recs, res, T, sres) == T
    torch.cuda.synchronize()
    assert launch_log(_abi.LOG_STREAM_RX_FRAME) == want_log
    assert _untouched(recs, 40, T) and _untouched(res, 16, T)
    out = ta.cpu().numpy()
    rc, rs = recs.cpu().numpy()[:T * 40].view(M.BATCH_REC), res.cpu().numpy()[:T * 16].view(M.BATCH_RES)
    sr = sres.cpu().numpy().view(S.STREAM_IN_RES)
    for i, (slot, data, ctr0, _) in enumerate(conns):
        want, wrecs, wbuf = O.stream_decrypt(c.ot[slot], data, ctr0.to_bytes(8, "big"), 0)
        g = sr[i]
        assert (int(g["status"]), int(g["nrec"]), int(g["consumed"]), bytes(g["in_ctr"])) == \
            (want["status"], want["nrec"], want["consumed"], want["in_ctr"]), i
        f = int(g["first"])
        for k, (off, doff, dlen, typ) in enumerate(wrecs):
            assert (int(rs[f + k]["data_offset"]), int(rs[f + k]["data_len"]), int(rs[f + k]["type"])) == \
                (doff, dlen, typ)
            s0 = offs[i] + off + doff
            assert int(rc[f + k]["buf_off"]) == offs[i] + off
            assert out[s0:s0 + dlen].tobytes() == wbuf[off + doff:off + doff + dlen], (i, k)
    c.close()
