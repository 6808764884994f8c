"""bench.py --dump-outputs: dump_outputs writes the results, the per-record
byte sums and a verbatim byte sample of the output arena as float32 .npy
files, over every record or -- past DUMP_PER_RECORD -- a sample that depends
on the seed alone.  Checked here on CPU tensors against numpy."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

torch = pytest.importorskip("torch")

N, STRIDE, LO, HI = 1000, 128, 8, 108


def _batch():
    import mbedtls_amd as M
    gen = torch.Generator()
    gen.manual_seed(7)
    arena = torch.randint(0, 256, (N * STRIDE,), dtype=torch.uint8, generator=gen)
    res = np.zeros(N, dtype=M.BATCH_RES)
    res["status"][5] = M.ERR_SSL_INVALID_MAC
    res["data_offset"] = np.arange(N)          # tells which record a dumped row is
    res["data_len"] = HI - LO
    res["type"] = 23
    return arena, torch.from_numpy(res.view(np.uint8).copy())


@pytest.mark.parametrize("cap", [1 << 21, 300])
def test_dump_outputs(tmp_path, monkeypatch, cap):
    monkeypatch.setattr(bench, "DUMP_PER_RECORD", cap)
    monkeypatch.setattr(bench, "DUMP_BYTES", 5000)
    arena, res = _batch()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arena, res, N, STRIDE, LO, HI)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["record_byte_sums.npy", "record_bytes.npy", "results.npy"]
    for f, a in got.items():
        assert a.dtype == np.float32
        assert np.array_equal(a, np.load(tmp_path / "b" / f)), f      # the sample does not change between runs
    r, sums, raw = got["results.npy"], got["record_byte_sums.npy"], got["record_bytes.npy"]
    k = min(N, cap)
    assert r.shape == (k, 4) and sums.shape == (k,) and raw.shape == (5000 // (HI - LO), HI - LO)
    ids = r[:, 1].astype(np.int64)
    assert np.all(np.diff(ids) > 0)
    if k == N:
        assert np.array_equal(ids, np.arange(N)) and r[5, 0] == -0x7180
    assert np.all(r[ids != 5, 0] == 0) and np.all(r[:, 2] == HI - LO) and np.all(r[:, 3] == 23)
    rows = arena.numpy().reshape(N, STRIDE)
    assert np.array_equal(sums, rows[ids, LO:HI].sum(axis=1))
    pick = ids[np.arange(raw.shape[0]) * k // raw.shape[0]]
    assert np.array_equal(raw, rows[pick, LO:HI])
