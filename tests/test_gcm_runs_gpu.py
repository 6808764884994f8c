"""The 8-wave wave passes (launch code -8; 2, 4, 16, 64 lanes) and the 16-wave
paired passes (-32; 2, 4, 8, 16, 32 lanes) of tlsrec_gcm_kernel on the inputs
its control flow branches on (tests/gcmrunlib.py): keys with no record and with
one, runs of R - 1 / R / R + 1 records that start anywhere in a wave's chunk
and cross a pair's chunk and a workgroup, several rounds per wave, block
counts m in {0, 1, L - 1, L, L + 1, 2 L, 2 L + 1}, and records that fail --
in their plan, in their tag, after it, or for want of a key -- in rounds they
share with good ones.

  (a) good records: every byte of both directions against OpenSSL EVP, every
      result field, one launch of the planned (L, code, tm) per direction;
  (b) one record in eight exceptional: those against the oracle, record by
      record (status, fields, the whole buffer in place), the others against
      EVP; no record is left out, and an unwritten result (zero) fails;
  (c) the stream and DTLS layers (records grouped by connection, no bucket
      pass) with 1 .. 40 records per connection.

Sizes follow the device's CU count.  Every comparison is bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests import gcmrunlib as G  # noqa: E402
from tests.batchlib import launch_log  # noqa: E402,F401  (fixture)
from tests.prng import prng_array  # noqa: E402
from tests.test_send_inplace_gpu import _assert_in_place, _check_dtls, _check_stream, _dtls_slots, dctr  # noqa: E402

CU = torch.cuda.get_device_properties(0).multi_processor_count
TABLE = G.case_table(CU)
IDS = list(TABLE)
DEV = torch.device("cuda")
SEEN = set()          # (L, code, cipher, decrypt) of every GCM launch (a) logged


def _env(monkeypatch, case):
    for v in G.SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def _table(b):
    kt = M.KeyTable(b.capacity)          # the last SPARE_SLOTS slots never hold a key
    kt.load(b.km)
    return kt


def _run(kt, case, d, arena, out, decrypt, log):
    """one batch call; returns (results, output arena) and checks the launch"""
    n = len(d)
    a = torch.from_numpy(arena).to(DEV)
    o = a if out is None else torch.zeros_like(a)
    res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)      # zero = a false success if left unwritten
    recs = torch.from_numpy(d.view(np.uint8).copy()).to(DEV)
    log.reset()
    (M.batch_decrypt if decrypt else M.batch_encrypt)(kt, recs, res, n, a, o, lanes=case.lanes, mean_bytes=case.hint)
    torch.cuda.synchronize()
    return res.cpu().numpy().view(M.BATCH_RES), o.cpu().numpy()


def _one_launch(log, case, sizing):
    assert log(_abi.LOG_BUCKET) == [(_abi.LOG_BUCKET, 1, 0, 0, 0)], log()
    gcm = log(_abi.LOG_GCM)
    assert gcm == [(_abi.LOG_GCM, case.L, case.code, sizing.tm, 0)], gcm
    assert not log(_abi.LOG_CHACHA) and not log(_abi.LOG_ALT_GCM) and not log(_abi.LOG_CCM)
    return gcm[0]


# ---- (a) good records -----------------------------------------------------------------
@pytest.mark.parametrize("cipher,ver", G.SUITES, ids=G.SUITE_IDS)
@pytest.mark.parametrize("cid", IDS)
def test_skewed_runs_vs_openssl_evp(cid, cipher, ver, monkeypatch, launch_log):
    case = TABLE[cid]
    _env(monkeypatch, case)
    s = case.runs
    # the plan the environment's switches give is the one the case was sized with
    p = _abi.gcm_plan(None, n=s.n, nloaded=s.nloaded, cu=CU, avg_bytes=case.hint, lanes=case.lanes, nr=G.NR[cipher],
                      has_cid=0, coalesced=0, keyrun=1)
    assert (p.L, p.code, p.rpw, p.tm) == (case.L, case.code, s.rpw, s.tm) and p.rpw >= min(3 * case.R, 64)
    b = G.RunBatch(case, s, cipher, ver, 1000 + cipher)
    kt = _table(b)
    try:
        # encrypt out of place
        r, got = _run(kt, case, b.desc(False), b.plain, "new", False, launch_log)
        e = _one_launch(launch_log, case, s)
        SEEN.add((e[1], e[2], cipher, False))
        assert (r["status"] == 0).all(), np.unique(r["status"], return_counts=True)
        assert (r["data_offset"] == 0).all() and (r["data_len"] == b.wire).all() and (r["type"] == 23).all()
        bad = b.evp(1, b.plain, got)
        assert int((bad != 0).sum()) == 0, f"{int((bad != 0).sum())} of {b.n} records differ from OpenSSL, " \
                                           f"first {np.flatnonzero(bad)[:5]} lengths {b.lens[np.flatnonzero(bad)[:5]]}"
        # decrypt EVP's seal in place
        r, got = _run(kt, case, b.desc(True), b.sealed(), None, True, launch_log)
        e = _one_launch(launch_log, case, s)
        SEEN.add((e[1], e[2], cipher, True))
        assert (r["status"] == 0).all(), np.unique(r["status"], return_counts=True)
        assert (r["data_offset"] == b.head).all() and (r["data_len"] == b.lens).all() and (r["type"] == 23).all()
        bad = b.evp(2, b.plain, got)
        assert int((bad != 0).sum()) == 0, f"{int((bad != 0).sum())} plaintexts differ, first " \
                                           f"{np.flatnonzero(bad)[:5]} lengths {b.lens[np.flatnonzero(bad)[:5]]}"
    finally:
        kt.close()


# ---- (b) bad records among good ones ------------------------------------------------------
def _check_mixed(b, d, before, ex, kinds, r, got, decrypt):
    """the exceptional records against the oracle one by one, the rest in bulk against EVP"""
    good = np.ones(b.n, bool)
    good[ex] = False
    statuses = []
    for k, i in zip(kinds, ex.tolist()):
        st, doff, dlen, typ, buf = b.oracle(decrypt, d, before, i)
        statuses.append(st)
        g = r[i]
        assert (int(g["status"]), int(g["data_offset"]), int(g["data_len"]), int(g["type"])) == \
            (st, doff, dlen, typ), (i, k, int(b.lens[i]), int(d["slot"][i]))
        o = int(b.off[i])
        assert got[o:o + len(buf)].tobytes() == buf, (i, k, int(b.lens[i]))
    gi = np.flatnonzero(good)
    assert len(gi) + len(ex) == b.n
    rg = r[gi]
    assert (rg["status"] == 0).all(), (np.unique(rg["status"], return_counts=True), gi[rg["status"] != 0][:5])
    if decrypt:
        assert (rg["data_offset"] == b.head).all() and (rg["data_len"] == b.lens[gi]).all()
    else:
        assert (rg["data_offset"] == 0).all() and (rg["data_len"] == b.wire[gi]).all()
    assert (rg["type"] == 23).all()
    bad = b.evp(2 if decrypt else 1, b.plain, got, sel=gi)
    assert int((bad != 0).sum()) == 0, f"{int((bad != 0).sum())} good records differ, first {gi[np.flatnonzero(bad)[:5]]}"
    return statuses


@pytest.mark.parametrize("cipher,ver", G.SUITES, ids=G.SUITE_IDS)
@pytest.mark.parametrize("cid", IDS)
def test_bad_records_among_good_ones(cid, cipher, ver, monkeypatch, launch_log):
    case = TABLE[cid]
    _env(monkeypatch, case)
    (bd, dd, arena, ex, kd), (be, de, plain, _, ke) = G.bad_batches(case, cipher, ver, 2000 + cipher)
    kt = _table(bd)
    try:
        r, got = _run(kt, case, dd, arena, None, True, launch_log)
        _one_launch(launch_log, case, case.thr)
        ds = _check_mixed(bd, dd, arena, ex, kd, r, got, True)
    finally:
        kt.close()
    kt = _table(be)
    try:
        r, got = _run(kt, case, de, plain, None, False, launch_log)
        _one_launch(launch_log, case, case.thr)
        es = _check_mixed(be, de, plain, ex, ke, r, got, False)
    finally:
        kt.close()
    assert G.coverage_ok(ver, ds, es)


# ---- (c) grouped order through the layers ---------------------------------------------------
def _conn_jobs(counts, seed, ctr_of):
    jobs = []
    for i, c in enumerate(counts.tolist()):
        jobs.append((i, prng_array(seed + i, c * 100 - i % 97).tobytes(), ctr_of(i), 100, 23))
    return jobs


def _paired_launch(log, dtls, send):
    if send:
        _assert_in_place(log, dtls=dtls)
    assert log(_abi.LOG_BUCKET) == [(_abi.LOG_BUCKET, 0, 0, 0, 0)], log()       # grouped: no bucket pass
    gcm = log(_abi.LOG_GCM)
    assert len(gcm) == 1 and gcm[0][2] == -32 and gcm[0][1] in (2, 4, 8) and gcm[0][3] == 31, gcm


def test_stream_connections_of_1_to_40_records(monkeypatch, launch_log):
    """AES-256-GCM on TLS 1.3, 100-byte fragments, send and receive"""
    for v in G.SWITCHES:
        monkeypatch.delenv(v, raising=False)
    counts = G.conn_counts(TABLE["pair-8"].runs.n)
    kl = M.KEYLEN[M.CIPHER_AES_256_GCM]
    raw = prng_array(7100, len(counts) * 48).reshape(-1, 48)
    c = B.Conns([(M.CIPHER_AES_256_GCM, M.VERSION_TLS1_3, raw[i, :kl].tobytes(), raw[i, 32:48].tobytes(), 0)
                 for i in range(len(counts))])
    try:
        jobs = _conn_jobs(counts, 71000, lambda i: 11 * i)
        launch_log.reset()
        got = c.encrypt(jobs, odd=True)
        _paired_launch(launch_log, False, True)
        assert [int(g[0]["nrec"]) for g in got] == counts.tolist()
        _check_stream(c, jobs, got)
        conns = [(slot, out, ctr, 0) for (slot, _, ctr, _, _), (_, out) in zip(jobs, got)]
        launch_log.reset()
        a, recs, res, sres, offs = c.decrypt(conns)
        _paired_launch(launch_log, False, False)
        for i, (slot, data, ctr, nbz) in enumerate(conns):
            g, pt = sres[i], jobs[i][1]
            assert (int(g["status"]), int(g["nrec"]), int(g["consumed"])) == (0, int(counts[i]), len(data)), i
            f, k = int(g["first"]), int(counts[i])
            assert (res["status"][f:f + k] == 0).all() and (res["type"][f:f + k] == 23).all(), i
            dl = res["data_len"][f:f + k]
            assert int(dl.sum()) == len(pt) and (dl[:-1] == 100).all(), i
            o = recs["buf_off"][f:f + k].astype(np.int64) + res["data_offset"][f:f + k]
            assert b"".join(a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, dl)) == pt, i
    finally:
        c.close()


def test_dtls_connections_of_1_to_40_records(monkeypatch, launch_log):
    """AES-128-GCM on DTLS 1.2, 100-byte fragments, send and receive (one record per datagram)"""
    for v in G.SWITCHES:
        monkeypatch.delenv(v, raising=False)
    counts = G.conn_counts(TABLE["pair-8"].runs.n)
    tab = B.Table(_dtls_slots(72, [M.CIPHER_AES_128_GCM], len(counts)))
    try:
        jobs = _conn_jobs(counts, 72000, lambda i: dctr(1 + i % 3, 7 * i))
        launch_log.reset()
        got = tab.encrypt(jobs, odd=True)
        _paired_launch(launch_log, True, True)
        assert [int(g[0]["nrec"]) for g in got] == counts.tolist()
        _check_dtls(tab, jobs, got)
        conns = []
        for (slot, pt, c8, frag, typ), (r, out, rc, rs) in zip(jobs, got):
            f, nrec = int(r["first"]), int(r["nrec"])
            starts = rc["buf_off"][f:f + nrec].astype(np.int64) - 13
            lens = 13 + rs["data_len"][f:f + nrec].astype(np.int64)
            grams = [out[int(s - starts[0]):int(s - starts[0] + ln)] for s, ln in zip(starts, lens)]
            assert b"".join(grams) == out
            conns.append((slot, {"in_epoch": int.from_bytes(c8[:2], "big")}, grams))
        launch_log.reset()
        rx = tab.decrypt(conns)
        _paired_launch(launch_log, True, False)
        B.check_vs_oracle(tab, conns, rx)
    finally:
        tab.close()


# ---- the families this module reached ---------------------------------------------------------
def test_all_nine_families_ran_for_both_key_sizes_and_directions():
    """after (a): a change of tlsrec_plan.h cannot turn a case into another
    family unnoticed (run with the whole module: it reads what (a) logged)"""
    assert {(L, code) for L, code, _, _ in SEEN} == G.FAMILY_CODES, sorted(SEEN)
    want = {(L, code, c, d) for L, code in G.FAMILY_CODES for c, _ in G.SUITES for d in (False, True)}
    assert SEEN == want, sorted(want - SEEN)
