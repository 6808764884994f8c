"""The inputs of tests/test_gcm_keypass_phase_gpu.py without a GPU
(tests/keypasslib.py): the record count and the batch call's arguments plan to
the 16-wave key passes at 8 and at 4 lanes on 64, 256 and 304 CUs, the lengths
hold every edge block count among the good and among the corrupted records
and one 16 383-byte record in every wave, and the oracle's expectation is
what the GPU test needs it to be -- its own seal opens to the content, a
corrupted tag gives INVALID_MAC and a wiped buffer."""
import numpy as np
import pytest

import mbedtls_amd as M
from tests import keypasslib as K

CUS = (64, 256, 304)
SMALL = 64                 # the oracle checks run on the smallest sizing


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("cipher,ver", K.SUITES, ids=K.SUITE_IDS)
@pytest.mark.parametrize("L", sorted(K.SHAPES))
def test_count_plans_to_the_key_passes(L, cipher, ver, cu):
    p = K.plan(cu, L, cipher)
    assert (p.L, p.code, p.waves, p.rpw, p.tm) == (L, 16, K.W, K.RPW, 1)
    if L == 8:
        assert p.g5 == 1                                 # the 5-bit Horner table (the G5 kernel exists at 8 lanes only)
    n = K.count(cu)
    assert p.grid == n // (K.W * K.RPW) + 1 and n % (K.W * K.RPW) == 1      # the last workgroup: one record


def test_the_hint_alone_does_not_reach_4_lanes_at_this_count():
    """why SHAPES[4] passes lanes = 4: the rule wants 16 records per wave of a full grid"""
    from mbedtls_amd import _abi
    from tests import gcmrunlib as G
    for cu in CUS:
        for n, want in ((K.count(cu), 8), (cu * 256, 4)):
            p = _abi.gcm_plan(G.default_knobs(), n=n, nloaded=1, cu=cu, avg_bytes=1400, lanes=0, nr=14, has_cid=0,
                              coalesced=0, keyrun=1)
            assert (p.L, p.code) == (want, 16)


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("ver", [M.VERSION_TLS1_2, M.VERSION_TLS1_3])
def test_lengths_meet_their_conditions(ver, cu):
    n = K.count(cu)
    lens = K.content_lengths(n, ver)
    aead = lens.astype(np.int64) + (1 if ver == M.VERSION_TLS1_3 else 0)
    m = (aead + 15) // 16
    bad = np.arange(n) % K.BAD_EVERY == K.BAD_AT
    for L in (8, 4):
        for want in (0, 1, L - 1, L, L + 1, 2 * L, 2 * L + 1):
            if want == 0 and ver == M.VERSION_TLS1_3:
                continue                                  # the inner type byte
            for d in (-1, 0, 1):
                v = 16 * want + d
                if v < (1 if ver == M.VERSION_TLS1_3 else 0):
                    continue
                assert int((aead[bad] == v).sum()) >= 2 and int((aead[~bad] == v).sum()) >= 8, (L, want, d)
            assert int((m == want).sum()) >= 16
    # one big record in every wave's positions, none elsewhere
    big = np.flatnonzero(lens == K.BIG)
    assert np.array_equal(big, K.big_positions(n))
    wave = (big // (K.W * K.RPW)) * K.W + big % K.W       # workgroup x 16 + wave of record i (identity order)
    full = n // (K.W * K.RPW)
    assert np.array_equal(np.sort(wave[big < full * K.W * K.RPW]), np.arange(full * K.W))
    assert int(bad[big].sum()) >= full and int((~bad[big]).sum()) >= full   # big ones fail and pass


@pytest.mark.parametrize("cipher,ver", K.SUITES, ids=K.SUITE_IDS)
def test_oracle_expectation(cipher, ver):
    b = K.batch(SMALL, cipher, ver)
    assert b.n == K.count(SMALL) and len(b.bad) * K.BAD_EVERY >= b.n - K.BAD_EVERY
    # encrypt: every record sealed, the wire layout of the suite
    assert (b.enc_want[:, 0] == 0).all() and (b.enc_want[:, 1] == 0).all()
    assert np.array_equal(b.enc_want[:, 2], b.wire.astype(np.int64)) and (b.enc_want[:, 3] == 23).all()
    # decrypt: the corrupted ones INVALID_MAC, the others the content again
    good = np.ones(b.n, bool)
    good[b.bad] = False
    assert (b.dec_want[b.bad, 0] == M.ERR_SSL_INVALID_MAC).all() and (b.dec_want[good, 0] == 0).all()
    assert np.array_equal(b.dec_want[good, 1], np.full(int(good.sum()), b.head))
    assert np.array_equal(b.dec_want[good, 2], b.lens[good].astype(np.int64)) and (b.dec_want[good, 3] == 23).all()
    for i in np.flatnonzero(good)[::97].tolist() + K.big_positions(b.n)[:4].tolist():
        if not good[i]:
            continue
        o, ln = int(b.off[i]) + b.head, int(b.lens[i])
        assert np.array_equal(b.dec_out[o:o + ln], b.plain[o:o + ln]), i
    # a failed record's output is wiped from the AEAD position on, and differs from its input there
    for i in b.bad[:64].tolist():
        o, size = int(b.off[i]), int(b.size[i])
        assert not b.dec_out[o + b.head:o + size].any(), i
        assert b.dec_in[o + b.head:o + size].any()
    # bytes between the record buffers belong to nobody
    assert b.total >= int(b.off[-1] + b.size[-1])
    # deterministic: the GPU test may share the cached batch
    assert K.batch(SMALL, cipher, ver) is b and not b.dec_out.flags.writeable
