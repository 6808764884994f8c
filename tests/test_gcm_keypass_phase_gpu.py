"""The 16-wave key passes of tlsrec_gcm_kernel (launch code 16) under one key,
at 8 lanes with the 5-bit Horner table and at 4 lanes, both directions,
AES-128-GCM on TLS 1.2 and AES-256-GCM on TLS 1.3, against the oracle record by
record (tests/keypasslib.py; its inputs are checked without a GPU in
tests/test_gcm_keypass_phase_cpu.py):

  * CUs x 128 + 1 records: every wave of a workgroup runs, for more than one
    round, and the last workgroup holds a single record;
  * block counts 0, 1, L - 1, L, L + 1, 2 L, 2 L + 1 (+- 1 byte) and one
    16 383-byte record in every wave, so waves of a workgroup leave the step
    loop at different times and run their tag stages beside stepping neighbours;
  * decrypt: one tag in eight corrupted -- INVALID_MAC and the wiped buffer
    next to records that pass.

Every result field of every record and every byte of the arena are compared;
the launch log shows the shape that ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402
from tests import gcmrunlib as G  # noqa: E402
from tests import keypasslib as K  # noqa: E402
from tests.batchlib import launch_log  # noqa: E402,F401  (fixture)

CU = torch.cuda.get_device_properties(0).multi_processor_count
DEV = torch.device("cuda")


@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
@pytest.mark.parametrize("L", sorted(K.SHAPES), ids=lambda L: f"L{L}")
@pytest.mark.parametrize("cipher,ver", K.SUITES, ids=K.SUITE_IDS)
def test_one_key_batch_vs_oracle(cipher, ver, L, decrypt, monkeypatch, launch_log):
    for v in G.SWITCHES:
        monkeypatch.delenv(v, raising=False)
    b = K.batch(CU, cipher, ver)
    args = K.SHAPES[L]
    p = _abi.gcm_plan(None, n=b.n, nloaded=1, cu=CU, avg_bytes=args["hint"], lanes=args["lanes"], nr=G.NR[cipher],
                      has_cid=0, coalesced=0, keyrun=1)
    assert (p.L, p.code, p.rpw) == (L, 16, K.RPW)
    assert L != 8 or p.g5 == 1                           # 8 lanes: the G5 kernel
    d, arena, want, out = (b.dec_desc, b.dec_in, b.dec_want, b.dec_out) if decrypt else \
        (b.enc_desc, b.plain, b.enc_want, b.enc_out)
    kt = M.KeyTable(1)
    try:
        kt.load(b.km)
        a = torch.from_numpy(arena.copy()).to(DEV)
        res = torch.zeros(b.n * 16, dtype=torch.uint8, device=DEV)       # zero = a false success if left unwritten
        recs = torch.from_numpy(d.view(np.uint8).copy()).to(DEV)
        launch_log.reset()
        (M.batch_decrypt if decrypt else M.batch_encrypt)(kt, recs, res, b.n, a, a, lanes=args["lanes"],
                                                          mean_bytes=args["hint"])
        torch.cuda.synchronize()
        gcm = launch_log(_abi.LOG_GCM)
        assert gcm == [(_abi.LOG_GCM, L, 16, p.tm, 0)], gcm
        assert not launch_log(_abi.LOG_CHACHA) and not launch_log(_abi.LOG_ALT_GCM) and not launch_log(_abi.LOG_CCM)
        r = res.cpu().numpy().view(M.BATCH_RES)
        got = a.cpu().numpy()
    finally:
        kt.close()
    fields = np.stack([r["status"].astype(np.int64), r["data_offset"].astype(np.int64),
                       r["data_len"].astype(np.int64), r["type"].astype(np.int64)], axis=1)
    diff = np.flatnonzero((fields != want).any(axis=1))
    assert len(diff) == 0, (len(diff), diff[:5], fields[diff[:5]], want[diff[:5]], b.lens[diff[:5]])
    assert (r["cid_len"] == 0).all()
    if decrypt:
        assert int((fields[:, 0] == M.ERR_SSL_INVALID_MAC).sum()) == len(b.bad)
    if not np.array_equal(got, out):
        at = np.flatnonzero(got != out)
        rec = np.searchsorted(b.off, at[:5].astype(np.uint64), side="right") - 1
        raise AssertionError(f"{len(at)} bytes differ from the oracle's, first in records {rec} of lengths {b.lens[rec]}")
