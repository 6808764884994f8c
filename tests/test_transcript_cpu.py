"""CPU-side checks of the transcript batch: the model of tests/transcript_ref.py
against hashlib, the layouts the binding shares with include/tlsrec.h, the order
of the call-level errors and the loud failure without a device."""
import hashlib
import os
import re

import numpy as np
import pytest

import mbedtls_amd as M
from mbedtls_amd import _abi
from mbedtls_amd import transcript as T
from tests import transcript_ref as R
from tests.prng import prng_bytes, splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASHES = [(R.ALG_SHA_256, hashlib.sha256, 32), (R.ALG_SHA_384, hashlib.sha384, 48)]
IDS = ["sha256", "sha384"]


def _cuts(seed, total):
    """a random segmentation of `total` bytes, empty pieces included"""
    s, cuts = seed, [0]
    while cuts[-1] < total:
        s, z = splitmix64(s)
        cuts.append(min(total, cuts[-1] + z % 97))
    return list(zip(cuts[:-1], cuts[1:])) or [(0, 0)]


@pytest.mark.parametrize("alg,H,hlen", HASHES, ids=IDS)
def test_model_matches_hashlib_for_every_length(alg, H, hlen):
    msg = prng_bytes(0x7115EC0DE, 300)
    for total in range(301):
        st = R.State()
        st.reset(alg)
        for lo, hi in _cuts(total * 7 + alg, total):
            st.update(msg[lo:hi])
            assert st.digest() == H(msg[:hi]).digest()          # a snapshot leaves the state running
        assert st.digest() == H(msg[:total]).digest() and len(st.digest()) == hlen
        assert st.count == total and st.hash == alg
        fill = total % (64 if hlen == 32 else 128)
        assert st.block == msg[total - fill:total] + bytes(128 - fill)
        assert R.State(st.to_bytes()).to_bytes() == st.to_bytes() and len(st.to_bytes()) == R.STATE_LEN


@pytest.mark.parametrize("alg,H,hlen", HASHES, ids=IDS)
def test_model_hrr(alg, H, hlen):
    m1, m2 = prng_bytes(1, 233), prng_bytes(2, 517)
    st = R.State()
    st.reset(alg)
    st.update(m1)
    st.hrr()
    assert st.count == 4 + hlen and st.block[:4] == b"\xfe\x00\x00" + bytes([hlen])
    st.update(m2)
    assert st.digest() == H(b"\xfe\x00\x00" + bytes([hlen]) + H(m1).digest() + m2).digest()


def test_model_batch_rules():
    arena, out = prng_bytes(3, 100), bytearray(b"\xaa" * 96)
    states = [bytes(R.STATE_LEN)] * 3
    segs = [(0, 0, 50, R.RESET | R.SNAPSHOT), (50, 48, 50, R.SNAPSHOT), (0, 0, 10, 0), (0, 0, 10, 8), (91, 0, 10, R.RESET),
            (0, 49, 0, R.RESET | R.SNAPSHOT)]
    conns = [(0, 0, 2, 0), (1, 2, 1, 0), (1, 3, 1, 0), (1, 4, 1, 0), (1, 5, 1, 0), (3, 0, 1, 0), (1, 5, 2, 0),
             (1, 0, 1, 1), (2, 0, 0, 0)]
    st = R.batch_update(R.ALG_SHA_256, states, conns, segs, arena, out)
    assert st == [0] + [R.BAD_INPUT_DATA] * 7 + [0]
    assert bytes(out[:32]) == hashlib.sha256(arena[:50]).digest() and bytes(out[32:48]) == bytes(16)
    assert bytes(out[48:80]) == hashlib.sha256(arena).digest()
    assert states[1] == states[2] == bytes(R.STATE_LEN)
    # a state of the other hash needs a RESET
    assert R.batch_update(R.ALG_SHA_384, states, [(0, 2, 1, 0)], segs, arena, out) == [R.BAD_INPUT_DATA]
    assert R.batch_update(R.ALG_SHA_256, states, [(0, 2, 1, 0)], segs, arena, out) == [0]


def test_layouts_and_constants():
    src = open(os.path.join(ROOT, "include", "tlsrec.h")).read()

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\w+?)u?\)?\s" % name, src).group(1), 0)

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out, off = [], 0
        for ctype, name, dim in re.findall(r"(uint64_t|uint32_t|uint8_t)\s+(\w+)(?:\[(\d+)\])?;", body):
            size = {"uint64_t": 8, "uint32_t": 4, "uint8_t": 1}[ctype]
            off = (off + size - 1) // size * size
            out.append((name, off, size * int(dim or 1)))
            off += size * int(dim or 1)
        return out, (off + 7) // 8 * 8

    assert define("TLSREC_TRANSCRIPT_RESET") == M.TRANSCRIPT_RESET == T.RESET == R.RESET == 1
    assert define("TLSREC_TRANSCRIPT_SNAPSHOT") == M.TRANSCRIPT_SNAPSHOT == T.SNAPSHOT == R.SNAPSHOT == 2
    assert define("TLSREC_TRANSCRIPT_HRR") == M.TRANSCRIPT_HRR == T.HRR == R.HRR == 4
    assert define("TLSREC_ALG_SHA_256") == M.ALG_SHA_256 == R.ALG_SHA_256
    assert define("TLSREC_ALG_SHA_384") == M.ALG_SHA_384 == R.ALG_SHA_384
    assert R.BAD_INPUT_DATA == M.ERR_SSL_BAD_INPUT_DATA
    for struct, dt in (("tlsrec_transcript_state", M.TRANSCRIPT_STATE), ("tlsrec_transcript_seg", M.TRANSCRIPT_SEG),
                       ("tlsrec_transcript_conn", M.TRANSCRIPT_CONN)):
        decl, size = fields(struct)
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == decl, struct
        assert dt.itemsize == size, struct
    assert M.TRANSCRIPT_STATE.itemsize == R.STATE_LEN == 208 and 208 % 16 == 0
    assert M.TRANSCRIPT_SEG.itemsize == 24 and M.TRANSCRIPT_CONN.itemsize == 16
    assert "tlsrec_transcript_batch_update" in _abi.SIGNATURES and hasattr(M.load(), "tlsrec_transcript_batch_update")


def test_call_level_errors_in_order():
    """each refusal with every later one also present, then each later one alone: no device is asked"""
    f = M.load().tlsrec_transcript_batch_update
    buf = np.zeros(256, dtype=np.uint8)
    p = buf.ctypes.data
    BAD = M.ERR_SSL_BAD_INPUT_DATA
    assert f(0, None, 0, None, 1, None, 1, None, 1, None, 1, None, None) == BAD                 # hash first
    assert f(0x02000008, p, 1, p, 0, p, 0, p, 0, p, 0, p, None) == BAD
    assert f(0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None) == BAD
    for alg in (M.ALG_SHA_256, M.ALG_SHA_384):
        for states, conns, status in ((None, p, p), (p, None, p), (p, p, None)):
            assert f(alg, states, 1, conns, 1, p, 1, p, 1, p, 48, status, None) == BAD
        assert f(alg, p, 1, p, 1, None, 1, p, 1, p, 48, p, None) == BAD
        assert f(alg, p, 1, p, 1, p, 1, None, 1, p, 48, p, None) == BAD
        assert f(alg, p, 1, p, 1, p, 1, p, 1, None, 48, p, None) == BAD
        # the later rules hold with nconns == 0 too; NULL arrays with zero counts are fine
        assert f(alg, None, 0, None, 0, None, 1, None, 0, None, 0, None, None) == BAD
        assert f(alg, None, 0, None, 0, None, 0, None, 1, None, 0, None, None) == BAD
        assert f(alg, None, 0, None, 0, None, 0, None, 0, None, 1, None, None) == BAD
        assert f(alg, None, 0, None, 0, None, 0, None, 0, None, 0, None, None) == 0
        assert f(alg, None, 5, None, 0, p, 1, p, 1, p, 48, None, None) == 0


def test_no_gpu_means_loud_failure():
    """Without a device a well-formed call is HW_ACCEL_FAILED, after the argument checks; no CPU hash."""
    L = M.load()
    if L.tlsrec_device_check() == 0:
        pytest.skip("a device is present")
    buf = np.zeros(256, dtype=np.uint8)
    p = buf.ctypes.data
    for alg in (M.ALG_SHA_256, M.ALG_SHA_384):
        assert L.tlsrec_transcript_batch_update(alg, p, 1, p, 1, p, 1, p, 1, p, 48, p, None) == M.ERR_SSL_HW_ACCEL_FAILED
        assert L.tlsrec_transcript_batch_update(alg, p, 1, p, 1, None, 1, p, 1, p, 48, p, None) == \
            M.ERR_SSL_BAD_INPUT_DATA
    assert not buf.any()
    with pytest.raises(Exception):
        T.new_states(1, "cuda")
