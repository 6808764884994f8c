"""The inputs of tests/test_gcm_runs_gpu.py without a GPU (tests/gcmrunlib.py):
every case plans to its kernel family with several rounds per wave on 64, 256
and 304 CUs, the generators meet the conditions they are there for, and the
two references -- OpenSSL EVP for the records in bulk, the oracle for the
exceptional ones -- agree byte for byte before either judges a kernel."""
import numpy as np
import pytest

import mbedtls_amd as M
from tests import gcmrunlib as G

CUS = (64, 256, 304)
IDS = list(G.case_table(64))
SMALL = G.case_table(64)          # the reference checks run on the smallest sizing


@pytest.mark.parametrize("cu", CUS)
def test_every_case_plans_to_its_family_with_several_rounds(cu):
    table = G.case_table(cu)
    assert {(c.L, c.code) for c in table.values()} == G.FAMILY_CODES
    for c in table.values():
        for nr in (10, 14):
            for s, rounds in ((c.runs, True), (c.thr, False)):
                p = c.plan(s.n, s.nloaded, nr)
                assert (p.L, p.code, p.rpw, p.tm) == (c.L, c.code, s.rpw, s.tm), (c.id, cu, nr)
                assert p.tm == (31 if c.code == -32 else 9) and p.waves == c.W
                assert not rounds or p.rpw >= min(3 * c.R, 64), (c.id, cu, p.rpw)
                assert p.grid > 1 and s.nloaded > 1
        assert c.thr.n % 8 == 0 and c.thr.n >= cu * c.W * c.R
        if c.band:
            for s in (c.runs, c.thr):
                assert c.band[0] <= s.n // s.nloaded < c.band[1]


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("cid", IDS)
def test_generators_meet_their_conditions(cid, cu):
    c = G.case_table(cu)[cid]
    for s, seed in ((c.runs, 11), (c.thr, 12)):
        idx = G.skewed_keyidx(s.nloaded, s.n, c.R, s.rpw, seed, c.W, c.band)      # asserts its own conditions
        assert idx.dtype == np.uint32 and len(idx) == s.n and int(idx.max()) < s.nloaded
        counts = np.bincount(idx, minlength=s.nloaded)
        assert int(counts.max()) > c.W * s.rpw and int((counts == 0).sum()) >= s.nloaded // 16
        assert np.array_equal(idx, G.skewed_keyidx(s.nloaded, s.n, c.R, s.rpw, seed, c.W, c.band))
        lens = G.edge_lengths(c.L, s.n, np.random.default_rng(seed))
        G.check_lengths(c.L, lens)
        m = (lens + 15) // 16
        for want in (0, 1, c.L - 1, c.L, c.L + 1, 2 * c.L, 2 * c.L + 1):
            assert int((m == want).sum()) >= 16, (cid, want)
        assert int((lens == 16383).sum()) == 16 and int(lens.max()) == 16383
        ex = G.exceptional(c.thr.n, seed)
        assert len(ex) * 8 == c.thr.n and len(np.unique(ex)) == len(ex)


@pytest.mark.parametrize("cipher,ver", G.SUITES, ids=G.SUITE_IDS)
@pytest.mark.parametrize("cid", IDS)
def test_evp_and_oracle_agree_on_a_slice(cid, cipher, ver):
    """512 records of the generated batch, spread over it: the oracle's seal
    of each equals EVP's wire bytes, and the oracle opens EVP's seal to the
    same content, fields and buffer."""
    b = G.RunBatch(SMALL[cid], SMALL[cid].runs, cipher, ver, 4000 + cipher)
    sel = np.unique(np.linspace(0, b.n - 1, 512).astype(np.int64))
    sealed = b.plain.copy()
    assert (b.evp(0, sealed, sel=sel, nthreads=2) == 0).all()
    de, dd = b.desc(False), b.desc(True)
    for i in sel.tolist():
        o, size, head, ln, wire = int(b.off[i]), int(b.size[i]), b.head, int(b.lens[i]), int(b.wire[i])
        st, doff, dlen, typ, buf = b.oracle(False, de, b.plain, i)
        assert (st, doff, dlen, typ) == (0, 0, wire, 23), i
        assert buf[:wire] == sealed[o:o + wire].tobytes(), (i, ln)
        st, doff, dlen, typ, buf = b.oracle(True, dd, sealed, i)
        assert (st, doff, dlen, typ) == (0, head, ln, 23), i
        assert buf[head:head + ln] == b.plain[o + head:o + head + ln].tobytes(), (i, ln)
    # the bulk comparison itself, on the same slice: EVP's check of the oracle's output
    got = b.plain.copy()
    for i in sel.tolist():
        o, size = int(b.off[i]), int(b.size[i])
        got[o:o + size] = np.frombuffer(b.oracle(False, de, b.plain, i)[4], dtype=np.uint8)
    assert (b.evp(1, b.plain, got, sel=sel, nthreads=2) == 0).all()
    got[int(b.off[sel[3]]) + b.head] ^= 1
    bad = b.evp(1, b.plain, got, sel=sel, nthreads=2)
    assert bad[3] != 0 and int((bad != 0).sum()) == 1, "the EVP check does not see a flipped byte"


@pytest.mark.parametrize("cipher,ver", G.SUITES, ids=G.SUITE_IDS)
@pytest.mark.parametrize("cid", IDS)
def test_exceptional_records_cover_the_statuses(cid, cipher, ver):
    """(b)'s condition on its inputs, on the oracle alone: the exceptional
    records of every case bring INVALID_MAC, BAD_INPUT_DATA, BUFFER_TOO_SMALL
    and (TLS 1.3) INVALID_RECORD, every kind occurs, and none of them passes."""
    (bd, dd, arena, ex, kd), (be, de, plain, _, ke) = G.bad_batches(SMALL[cid], cipher, ver, 5000 + cipher)
    assert len(ex) * 8 == bd.n
    assert set(kd) == {k for k in G.DEC_KINDS if k != "zero-inner" or ver == M.VERSION_TLS1_3}
    assert set(ke) == set(G.ENC_KINDS)
    ds = [bd.oracle(True, dd, arena, i)[0] for i in ex.tolist()]
    es = [be.oracle(False, de, plain, i)[0] for i in ex.tolist()]
    assert G.coverage_ok(ver, ds, es)
    by = {}
    for k, s in list(zip(kd, ds)) + list(zip(ke, es)):
        by.setdefault(k, set()).add(s)
    assert by["tag-bit"] == by["ct-bit"] == by["type"] == by["len-1"] == by["short"] == {M.ERR_SSL_INVALID_MAC}
    assert by["slot-unloaded"] == by["slot-past"] == by["len-16385"] == {M.ERR_SSL_BAD_INPUT_DATA}
    assert by["buf-short"] == {M.ERR_SSL_BUFFER_TOO_SMALL}
    assert ver != M.VERSION_TLS1_3 or by["zero-inner"] == {M.ERR_SSL_INVALID_RECORD}
    # the good seven in eight are untouched by the spoiling
    good = np.ones(bd.n, bool)
    good[ex] = False
    assert np.array_equal(dd[good], bd.desc(True)[good]) and np.array_equal(de[good], be.desc(False)[good])
