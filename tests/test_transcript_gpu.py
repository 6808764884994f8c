"""GPU parity of tlsrec_transcript_batch_update with the model of
tests/transcript_ref.py: after every call the snapshot arena, the status array
and the full state bytes in device memory equal the model's, bit for bit, with
canaries around everything the call may write; then three chains in which the
snapshots feed the existing batch calls without passing through the host."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402
from mbedtls_amd import keysched as K  # noqa: E402
from mbedtls_amd import tls12 as T12  # noqa: E402
from mbedtls_amd import transcript as T  # noqa: E402
from tests import tls12_hs_ref as R12  # noqa: E402
from tests import tls13_early_ref as RE  # noqa: E402
from tests import tls13_ref as R13  # noqa: E402
from tests import transcript_ref as R  # noqa: E402
from tests.prng import prng_bytes, splitmix64  # noqa: E402

DEV = torch.device("cuda")
HASHES = [(R.ALG_SHA_256, "sha256"), (R.ALG_SHA_384, "sha384")]
IDS = ["sha256", "sha384"]
HL = {"sha256": 32, "sha384": 48}
RS, SN, HR = R.RESET, R.SNAPSHOT, R.HRR
BAD, CANARY, GUARD = M.ERR_SSL_BAD_INPUT_DATA, 0xA5, 64


def _t(raw):
    return torch.from_numpy(np.frombuffer(bytes(raw), dtype=np.uint8).copy()).to(DEV)


def _guarded(raw, shift=0):
    """`raw` on the device between canaries, `shift` bytes past a 16-byte boundary"""
    buf = torch.full((GUARD + shift + len(raw) + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + len(raw)]
    if len(raw):
        view.copy_(_t(raw))
    assert buf.data_ptr() % 16 == 0
    return buf, view


def _read(buf, view, shift=0):
    raw = buf.cpu().numpy().tobytes()
    lo = GUARD + shift
    assert raw[:lo] == bytes([CANARY]) * lo and raw[lo + view.numel():] == bytes([CANARY]) * GUARD, "guard bytes"
    return raw[lo:lo + view.numel()]


def run(alg, states, conns, segs, arena, out_len, out_fill=None, shift=0):
    """one call on the device and in the model over the same inputs; compares status,
    snapshots and every state, checks canaries and that arena is unchanged.
    `states` (list of 208-byte states) is advanced in place; returns (status, out)."""
    out0 = bytes([CANARY]) * out_len if out_fill is None else out_fill
    sbuf, sview = _guarded(b"".join(states))
    abuf, aview = _guarded(arena, shift)
    obuf, oview = _guarded(out0, shift)
    stbuf, stview = _guarded(bytes(4 * len(conns)))
    c = np.array([tuple(x) for x in conns], dtype=M.TRANSCRIPT_CONN).reshape(-1)
    s = np.array([tuple(x) for x in segs], dtype=M.TRANSCRIPT_SEG).reshape(-1)
    keep = T.batch_update(alg, sview, c, s, aview, oview, stview.view(torch.int32), nstates=len(states))
    torch.cuda.synchronize()
    del keep
    model_out = bytearray(out0)
    want = R.batch_update(alg, states, [tuple(x) for x in conns], [tuple(x) for x in segs], bytes(arena), model_out)
    got_status = list(np.frombuffer(_read(stbuf, stview), dtype=np.int32))
    assert got_status == want, "status"
    got_out = _read(obuf, oview, shift)
    assert got_out == bytes(model_out), "snapshots"
    got_states = _read(sbuf, sview)
    for i, st in enumerate(states):
        assert got_states[208 * i:208 * i + 208] == st, f"state {i}"
    assert _read(abuf, aview, shift) == bytes(arena), "arena"
    return want, got_out


def _fresh(n):
    return [bytes(R.STATE_LEN)] * n


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_padding_edges(alg, hname):
    lens = [0, 1, 55, 56, 57, 63, 64, 65, 111, 112, 113, 119, 120, 127, 128, 129, 239, 240, 255, 256, 257, 1000, 4099]
    arena, segs, off = prng_bytes(0x7A01, sum(lens) + len(lens)), [], 0
    for i, n in enumerate(lens):
        segs.append((off, 48 * i, n, RS | SN))
        off += n + 1
    states = _fresh(len(lens))
    st, out = run(alg, states, [(i, i, 1, 0) for i in range(len(lens))], segs, arena, 48 * len(lens))
    assert st == [0] * len(lens)
    H = HL[hname]
    for i, (n, sg) in enumerate(zip(lens, segs)):
        d = hashlib.new(hname, arena[sg[0]:sg[0] + n]).digest()
        assert out[48 * i:48 * i + 48] == d + bytes(48 - H), n


def _cut_case(msg, seed):
    """201 connections: the message cut in two at every byte, the first piece at an arena
    offset = cut mod 16 (mod 16), the second at an unrelated odd offset"""
    arena, first, second = bytearray(), [], []
    s = seed
    for cut in range(len(msg) + 1):
        arena += bytes(-len(arena) % 16) + bytes(cut % 16)
        first.append((len(arena), 0, cut, RS))
        arena += msg[:cut]
        s, z = splitmix64(s)
        arena += bytes(1 + z % 13)
        if len(arena) % 2 == 0:
            arena += b"\x00"
        second.append((len(arena), 48 * cut, len(msg) - cut, SN))
        arena += msg[cut:]
    assert all(f[0] % 16 == c % 16 for c, f in enumerate(first)) and all(x[0] % 2 == 1 for x in second)
    return bytes(arena), first, second


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_every_phase_in_one_call(alg, hname):
    msg = prng_bytes(0x7A02, 200)
    arena, first, second = _cut_case(msg, 5)
    n = len(first)
    segs = [x for pair in zip(first, second) for x in pair]
    st, out = run(alg, _fresh(n), [(i, 2 * i, 2, 0) for i in range(n)], segs, arena, 48 * n)
    d = hashlib.new(hname, msg).digest()
    assert st == [0] * n and all(out[48 * i:48 * i + len(d)] == d for i in range(n))


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_carry_across_calls(alg, hname):
    msg = prng_bytes(0x7A03, 200)
    arena, first, second = _cut_case(msg, 6)
    n = len(first)
    states = _fresh(n)
    run(alg, states, [(i, i, 1, 0) for i in range(n)], first, arena, 0)
    assert all(R.State(s).count == i for i, s in enumerate(states))
    st, out = run(alg, states, [(i, i, 1, 0) for i in range(n)], second, arena, 48 * n)
    d = hashlib.new(hname, msg).digest()
    assert st == [0] * n and all(out[48 * i:48 * i + len(d)] == d for i in range(n))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_counts(alg, hname, count):
    arena = prng_bytes(0x7A04 + count, 3 + 150 * count)
    segs = [(3 + 150 * i, 48 * i, 150 - (i % 5), RS | SN) for i in range(count)]
    st, _ = run(alg, _fresh(count), [(i, i, 1, 0) for i in range(count)], segs, arena, 48 * count)
    assert st == [0] * count


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_divergent_trip_counts(alg, hname):
    count = 130
    lens = [(3000 * i) // (count - 1) for i in range(count)]
    s = 11
    for i in range(count - 1, 0, -1):                # Fisher-Yates
        s, z = splitmix64(s)
        j = z % (i + 1)
        lens[i], lens[j] = lens[j], lens[i]
    assert min(lens) == 0 and max(lens) == 3000
    arena = prng_bytes(0x7A05, sum(lens) + 2 * count + 1)
    segs, off = [], 1
    for i, n in enumerate(lens):
        segs.append((off, 48 * i, n, RS | SN))
        off += n + (i % 3)
    st, _ = run(alg, _fresh(count), [(i, i, 1, 0) for i in range(count)], segs, arena, 48 * count)
    assert st == [0] * count


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_snapshots_and_zero_length_segments(alg, hname):
    H = HL[hname]
    arena = prng_bytes(0x7A06, 700)
    cuts = [0, 130, 131, 460, 697]
    segs = [(cuts[k] + 1, 48 * k, cuts[k + 1] - cuts[k], (RS if k == 0 else 0) | SN) for k in range(4)]
    segs += [(1, 0, 130, RS), (131, 0, 1, 0), (132, 0, 329, 0), (461, 192, 237, SN)]       # no snapshots on the way
    segs += [(700, 240, 0, RS | SN), (5, 288, 0, SN), (0, 0, 0, HR), (0, 336, 0, SN)]
    conns = [(0, 0, 4, 0), (1, 4, 4, 0), (2, 8, 1, 0), (0, 9, 1, 0), (3, 10, 2, 0)]
    states = _fresh(4)
    # one connection per state and call: state 0's second visit is a second call
    st, out = run(alg, states, conns[:3], segs, arena, 384)
    assert st == [0, 0, 0]
    for k in range(4):
        assert out[48 * k:48 * k + H] == hashlib.new(hname, arena[1:1 + cuts[k + 1]]).digest()
    assert out[192:240] == out[144:192] and states[0] == states[1]
    assert out[240:240 + H] == hashlib.new(hname, b"").digest()
    states[3] = states[0]
    st, out2 = run(alg, states, conns[3:], segs, arena, 384, out_fill=out)
    assert st == [0, 0] and out2[288:336] == out[144:192]
    hrr = hashlib.new(hname, b"\xfe\x00\x00" + bytes([H]) + out[144:144 + H]).digest()
    assert out2[336:336 + H] == hrr


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_hrr_then_continue_and_reset_in_the_middle(alg, hname):
    H = HL[hname]
    ch1, hrr_ch2, other = prng_bytes(1, 517), prng_bytes(2, 88 + 611), prng_bytes(3, 77)
    arena = b"\x00" + ch1 + b"\x00\x00" + hrr_ch2 + other
    o1, o2, o3 = 1, 1 + 517 + 2, 1 + 517 + 2 + len(hrr_ch2)
    segs = [(o1, 0, 517, RS | HR), (o2, 0, len(hrr_ch2), SN),
            (o1, 48, 517, RS | SN), (o3, 96, 77, RS | SN), (o1, 144, 100, SN)]
    st, out = run(alg, _fresh(2), [(0, 0, 2, 0), (1, 2, 3, 0)], segs, arena, 192)
    assert st == [0, 0]
    assert out[:H] == hashlib.new(hname, b"\xfe\x00\x00" + bytes([H]) + hashlib.new(hname, ch1).digest() +
                                  hrr_ch2).digest()
    assert out[96:96 + H] == hashlib.new(hname, other).digest()
    assert out[144:144 + H] == hashlib.new(hname, other + ch1[:100]).digest()


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_clone_continues_identically(alg, hname):
    arena = prng_bytes(0x7A08, 1000)
    states = T.new_states(2, DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.zeros(96, dtype=torch.uint8, device=DEV)
    c = np.array([(0, 0, 1, 0)], dtype=M.TRANSCRIPT_CONN)
    s = np.array([(3, 0, 333, RS)], dtype=M.TRANSCRIPT_SEG)
    keep = [T.batch_update(alg, states, c, s, _t(arena), None, status[:1])]
    states[1].copy_(states[0])                     # the clone: a device copy of 208 bytes
    c = np.array([(0, 0, 1, 0), (1, 1, 1, 0)], dtype=M.TRANSCRIPT_CONN)
    s = np.array([(336, 0, 500, SN), (336, 48, 500, SN)], dtype=M.TRANSCRIPT_SEG)
    keep.append(T.batch_update(alg, states, c, s, _t(arena), out, status))
    torch.cuda.synchronize()
    raw, o = states.cpu().numpy().tobytes(), out.cpu().numpy().tobytes()
    assert raw[:208] == raw[208:] and o[:48] == o[48:] and status.tolist() == [0, 0]
    assert o[:HL[hname]] == hashlib.new(hname, arena[3:836]).digest()


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_long_count(alg, hname):
    """a crafted state just below 2^32 bytes: the padding's length word is 64 bits wide"""
    st = R.State()
    st.reset(alg)
    bits = 32 if hname == "sha256" else 64
    words = np.frombuffer(prng_bytes(0x7A09, 64), dtype="<u8")
    st.h = [int(x) & ((1 << bits) - 1) for x in words]
    st.count = 2 ** 32 - 37
    fill = st.count % (2 * bits)
    st.block = prng_bytes(0x7A0A, fill) + bytes(128 - fill)
    states = [st.to_bytes()]
    arena = prng_bytes(0x7A0B, 203)
    status, out = run(alg, states, [(0, 0, 1, 0)], [(3, 0, 200, SN)], arena, 48)
    assert status == [0] and R.State(states[0]).count == 2 ** 32 + 163
    twin = R.State(st.to_bytes())
    twin.count -= 2 ** 32 - 2 ** 10              # the same state but for a short count: another digest
    twin.update(arena[3:])
    assert twin.digest() != out[:HL[hname]]


@pytest.mark.parametrize("shift", [0, 1, 7])
@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_output_placement_and_untouched_memory(alg, hname, shift):
    """elements at 16-aligned and odd addresses with canaries between them; states the
    call does not name, the arena and the guards of every array stay as they were"""
    H, n = HL[hname], 6
    arena = prng_bytes(0x7A0C + shift, 902)          # the last segment ends on the arena's last byte
    offs = [0, 49, 112, 161 + 8, 224 + 9, 300]      # gaps of 1..28 canary bytes between the elements
    segs = [(7 + 150 * i, offs[i], 140 + i, RS | SN) for i in range(n)]
    other = R.State()
    other.reset(alg)
    other.update(b"unnamed state")
    states = [bytes(208), other.to_bytes(), bytes(208), bytes([0xEE]) * 208] + _fresh(n)
    named = [4, 6, 0, 2, 8, 9]
    st, out = run(alg, states, [(named[i], i, 1, 0) for i in range(n)], segs, arena, 349, shift=shift)
    assert st == [0] * n
    assert states[1] == other.to_bytes() and states[3] == bytes([0xEE]) * 208 and states[5] == states[7] == bytes(208)
    covered = set()
    for i in range(n):
        assert out[offs[i] + H:offs[i] + 48] == bytes(48 - H)
        covered |= set(range(offs[i], offs[i] + 48))
    assert all(out[k] == CANARY for k in range(349) if k not in covered)


ERRORS = {
    "state_past_nstates": dict(conn=(5, 1, 1, 0)),
    "segs_past_nsegs": dict(conn=(1, 6, 2, 0)),
    "first_seg_overflow": dict(conn=(1, 0xFFFFFFFF, 2, 0)),
    "reserved": dict(conn=(1, 1, 1, 7)),
    "unknown_flag": dict(seg=(10, 48, 20, RS | SN | 8)),
    "arena_end": dict(seg=(581, 48, 20, RS | SN)),
    "off_overflow": dict(seg=(2 ** 64 - 4, 48, 20, RS | SN)),
    "snapshot_past_out": dict(seg=(10, 240 - 47, 20, RS | SN)),
    "out_off_overflow": dict(seg=(10, 2 ** 64 - 16, 20, RS | SN)),
    "hash_mismatch_zeroed": dict(seg=(10, 48, 20, SN)),
    "hash_mismatch_other": dict(seg=(10, 48, 20, SN), other=True),
    "bad_second_segment": dict(conn=(1, 5, 2, 0)),
}


@pytest.mark.parametrize("rule", sorted(ERRORS))
@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_per_connection_errors(alg, hname, rule):
    """connection 1 breaks one rule among four good ones: its state and snapshot bytes stay
    as they were (the model leaves them and run() compares all of both arrays)"""
    e = ERRORS[rule]
    arena = prng_bytes(0x7A0D, 600)
    segs = [(100 * i + 1, 48 * i, 90 + i, RS | SN) for i in range(5)]
    segs += [(300, 48, 64, RS | SN), (590, 48, 11, SN)]       # 5, 6: a good segment, then one past the arena
    if "seg" in e:
        segs[1] = e["seg"]
    conns = [(i, i, 1, 0) for i in range(5)]
    if "conn" in e:
        conns[1] = e["conn"]
    states = _fresh(5)
    if e.get("other"):
        st = R.State()
        st.reset(R.ALG_SHA_384 if alg == R.ALG_SHA_256 else R.ALG_SHA_256)
        st.update(b"a state of the other hash")
        states[1] = st.to_bytes()
    before = states[1]
    status, out = run(alg, states, conns, segs, arena, 240)
    assert status == [0, BAD, 0, 0, 0]
    assert states[1] == before and out[48:96] == bytes([CANARY]) * 48
    for i in (0, 2, 3, 4):
        assert out[48 * i:48 * i + HL[hname]] == hashlib.new(hname, arena[100 * i + 1:100 * i + 91 + i]).digest()


def test_status_rows_of_the_call_only():
    """nconns == 0 launches nothing; otherwise exactly status[0 .. nconns) is written"""
    status = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    states = T.new_states(1, DEV)
    f = M.load().tlsrec_transcript_batch_update
    assert f(M.ALG_SHA_256, states.data_ptr(), 1, None, 0, None, 0, None, 0, None, 0, status.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [77] * 4
    c = _t(np.array([(0, 0, 0, 0), (0, 0, 0, 1)], dtype=M.TRANSCRIPT_CONN).tobytes())
    assert f(M.ALG_SHA_256, states.data_ptr(), 1, c.data_ptr(), 2, None, 0, None, 0, None, 0,
             status[1:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [77, 0, BAD, 77]


# ---- the snapshots feed the next batch call, nothing staged through the host ----
def _messages(seed, count, lo, hi):
    out, s = [], seed
    for i in range(count):
        s, z = splitmix64(s)
        out.append(prng_bytes(seed * 1000 + i, lo + z % (hi - lo)))
    return out


def _arena(msgs):
    """the messages back to back with one odd gap each; returns (bytes, offsets)"""
    buf, offs = bytearray(b"\x00"), []
    for i, m in enumerate(msgs):
        offs.append(len(buf))
        buf += m + bytes(1 + i % 2)
    return bytes(buf), offs


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_chain_tls13_handshake_keys(alg, hname):
    count, first, H = 65, 1, HL[hname]
    cipher = M.CIPHER_AES_128_GCM if hname == "sha256" else M.CIPHER_AES_256_GCM
    msgs = _messages(41, count, 300, 900)                     # ClientHello || ServerHello
    arena, offs = _arena(msgs)
    raw = bytearray(prng_bytes(0x7A10, count * 176))
    for i in range(count):
        raw[176 * i + 128:176 * i + 176] = bytes([0xCC]) * 48       # the transcript fields: not yet known
    conns = _t(raw)
    c = np.array([(i, i, 1, 0) for i in range(count)], dtype=M.TRANSCRIPT_CONN)
    s = np.array([(offs[i], 176 * i + 128, len(msgs[i]), RS | SN) for i in range(count)], dtype=M.TRANSCRIPT_SEG)
    states, status = T.new_states(count, DEV), torch.zeros(count, dtype=torch.int32, device=DEV)
    hs = torch.zeros(2 * count * 48, dtype=torch.uint8, device=DEV)
    ms = torch.zeros(count * 48, dtype=torch.uint8, device=DEV)
    kt = M.KeyTable(first + 2 * count)
    keep = T.batch_update(alg, states, c, s, _t(arena), conns, status)
    K.keytab_derive_handshake(kt, first, count, cipher, 32, 32, conns, hs, None, ms)
    torch.cuda.synchronize()
    del keep
    assert status.tolist() == [0] * count
    hs, ms = hs.cpu().numpy().tobytes(), ms.cpu().numpy().tobytes()
    for i in range(count):
        tr = hashlib.new(hname, msgs[i]).digest()
        want = R13.handshake_stage(hname, bytes(raw[176 * i:176 * i + 32]), bytes(raw[176 * i + 48:176 * i + 80]), tr,
                                   M.KEYLEN[cipher])
        assert hs[96 * i:96 * i + H] == want["c_hs"] and hs[96 * i + 48:96 * i + 48 + H] == want["s_hs"], i
        assert ms[48 * i:48 * i + H] == want["master"], i
    kt.close()


@pytest.mark.parametrize("alg,hname", HASHES, ids=IDS)
def test_chain_tls13_psk_binders(alg, hname):
    count, H = 66, HL[hname]
    hellos = _messages(43, count, 200, 700)
    blens = [3 + H for _ in hellos]                           # binders list: 2 + (1 + Hash.length)
    psks = [prng_bytes(0x7A20 + i, 32) for i in range(count)]
    offered = []
    for i, m in enumerate(hellos):
        trunc = m[:len(m) - blens[i]]
        offered.append(RE.early_stage(hname, psks[i], True, hashlib.new(hname, trunc).digest(),
                                      hashlib.new(hname, m).digest(), 16)["binder"])
    wire = [bytearray(m) for m in hellos]
    flipped = set(range(1, count, 3))
    for i in flipped:
        wire[i][(7 * i) % (len(wire[i]) - blens[i])] ^= 0x10   # one bit of the truncated ClientHello
    arena, offs = _arena([bytes(w) for w in wire])
    raw = bytearray(count * 144)
    for i in range(count):
        raw[144 * i:144 * i + 32] = psks[i]
        raw[144 * i + 48:144 * i + 144] = bytes([0xCC]) * 96
    conns = _t(raw)
    c = np.array([(i, 2 * i, 2, 0) for i in range(count)], dtype=M.TRANSCRIPT_CONN)
    s = np.zeros(2 * count, dtype=M.TRANSCRIPT_SEG)
    for i in range(count):
        cut = len(wire[i]) - blens[i]
        s[2 * i] = (offs[i], 144 * i + 48, cut, RS | SN)                   # -> binder_transcript
        s[2 * i + 1] = (offs[i] + cut, 144 * i + 96, blens[i], SN)         # -> hello_transcript
    states, status = T.new_states(count, DEV), torch.zeros(count, dtype=torch.int32, device=DEV)
    off_t = _t(b"".join(o + bytes(48 - H) for o in offered))
    match = torch.full((count,), 9, dtype=torch.int32, device=DEV)
    keep = T.batch_update(alg, states, c, s, _t(arena), conns, status)
    K.batch_psk_binder(alg, 32, K.PSK_RESUMPTION, conns, off_t, None, match, count)
    torch.cuda.synchronize()
    del keep
    assert status.tolist() == [0] * count
    assert match.tolist() == [0 if i in flipped else 1 for i in range(count)]
    got = conns.cpu().numpy().tobytes()
    for i in range(count):
        assert got[144 * i + 96:144 * i + 96 + H] == hashlib.new(hname, bytes(wire[i])).digest()


def test_chain_tls12_finished_sha384():
    count, hname = 70, "sha384"
    msgs = _messages(47, count, 1500, 2600)                   # a whole TLS 1.2 handshake up to the Finished
    arena, offs = _arena(msgs)
    raw = prng_bytes(0x7A30, count * 112)
    conns = _t(raw)
    trs = torch.full((count * 48,), 0xCC, dtype=torch.uint8, device=DEV)
    c = np.array([(i, i, 1, 0) for i in range(count)], dtype=M.TRANSCRIPT_CONN)
    s = np.array([(offs[i], 48 * i, len(msgs[i]), RS | SN) for i in range(count)], dtype=M.TRANSCRIPT_SEG)
    states, status = T.new_states(count, DEV), torch.zeros(count, dtype=torch.int32, device=DEV)
    verify = torch.zeros(count * 16, dtype=torch.uint8, device=DEV)
    keep = T.batch_update(R.ALG_SHA_384, states, c, s, _t(arena), trs, status)
    T12.tls12_batch_verify_data(_abi.TLS_PRF_SHA384, _abi.IS_CLIENT, conns, trs, None, verify, None, count)
    torch.cuda.synchronize()
    del keep
    assert status.tolist() == [0] * count
    v = verify.cpu().numpy().tobytes()
    for i in range(count):
        want = R12.verify_data(hname, raw[112 * i:112 * i + 48], hashlib.sha384(msgs[i]).digest(), _abi.IS_CLIENT)
        assert v[16 * i:16 * i + 12] == want, i
