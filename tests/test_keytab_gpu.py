"""The key table's loads and its bookkeeping (mbedtls_amd/csrc/keytab.hip), on tables of 4 slots and at most 4
records of 64 bytes: host and device-resident AEAD material load alike, an AEAD key over a CBC slot, a bad
record that leaves the table as it was, and an engine slot freed and allocated again.  Every record is compared
with the oracle (AEAD) or the record model of tests/cbc_ref.py (CBC)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
import oracle as O  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402
from mbedtls_amd import cbc as C  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests import cbc_ref as R  # noqa: E402
from tests import cbclib as L  # noqa: E402
from tests.prng import prng_bytes  # noqa: E402

DEV = torch.device("cuda")


def _slot_cipher(kt, slot):
    f = _abi.load().tlsrec__keytab_cipher
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint32], ctypes.c_int
    return f(kt.handle, slot)


def _has_cbc(kt):
    f = _abi.load().tlsrec__keytab_has_cbc
    f.argtypes, f.restype = [ctypes.c_void_p], ctypes.c_int
    return f(kt.handle)


def _sealed(recs, want):
    return [B.Rec(r.slot, bytearray(w[5]), w[1], w[2], r.ctr, w[3], r.ver) for r, w in zip(recs, want)]


def test_host_and_device_resident_aead_material_load_alike():
    """AES-128-GCM material from a numpy array and from a device tensor: the same 4 records encrypt to the same
    bytes under each table, the oracle's"""
    slots = B.random_slots(61, [M.CIPHER_AES_128_GCM], [M.VERSION_TLS1_2, M.VERSION_TLS1_3], 4)
    batch = B.Batch(slots, B.plaintext_records(slots, [64, 63, 1, 64], seed=9))
    km = batch.key_materials()
    outs = []
    for on_device in (False, True):
        kt = M.KeyTable(4)
        kt.load(torch.from_numpy(km.view(np.uint8).copy()).to(DEV) if on_device else km)
        assert [_slot_cipher(kt, s) for s in range(4)] == [M.CIPHER_AES_128_GCM] * 4
        out, res = batch.run_gpu(False, kt=kt)
        bad = batch.compare(False, out, res)
        assert not bad, (on_device, bad[:3])
        outs.append((out, res))
        kt.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_aead_key_over_a_cbc_slot():
    """slot 0 held AES-128-CBC + SHA-256 and is loaded again with AES-256-GCM (the key setup behind the CBC wipe):
    its records match the oracle both ways, its CBC neighbour still matches the model, and the table still counts
    as one that has held CBC slots"""
    cbc = [L.make_key(70 + i, R.CIPHER_AES_128_CBC, R.MAC_SHA256, i) for i in range(2)]
    kt = L.load_table(cbc)
    assert _has_cbc(kt) == 1
    aead = B.random_slots(71, [M.CIPHER_AES_256_GCM], [M.VERSION_TLS1_2], 1)[0]
    kt.load(M.key_material(*aead), first=0)
    assert [_slot_cipher(kt, s) for s in range(2)] == [M.CIPHER_AES_256_GCM, R.CIPHER_AES_128_CBC]
    assert _has_cbc(kt) == 1
    slots = [aead, cbc[1]]
    recs = [L.plain_rec(i % 2, n, 300 + i, head=24) for i, n in enumerate([64, 64, 17, 0])]
    run = L.Run(slots, recs)
    want = run.expected(False)
    assert all(w[0] == 0 for w in want)
    out, res = run.gpu(False, kt=kt)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:3]
    back = L.Run(slots, _sealed(recs, want))
    out, res = back.gpu(True, kt=kt)
    bad = back.compare(True, out, res)
    assert not bad, bad[:3]
    kt.close()


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("kind", ["aead", "cbc"])
def test_a_bad_record_leaves_the_table_unchanged(kind, on_device):
    """three records, the last one bad (a tag length its cipher does not have; etm = 2): the documented error,
    and no slot of the three counts as loaded"""
    lib = _abi.load()
    kt = M.KeyTable(4)
    if kind == "aead":
        slots = B.random_slots(81, [M.CIPHER_AES_128_GCM, M.CIPHER_CHACHA20_POLY1305], [M.VERSION_TLS1_3], 3)
        km = np.concatenate([M.key_material(*s) for s in slots])
        km["taglen"][2] = 8
        fn, want = lib.tlsrec_keytab_load, M.ERR_SSL_FEATURE_UNAVAILABLE
    else:
        keys = [L.make_key(82 + i, R.CIPHER_AES_128_CBC, R.MAC_SHA1, 0) for i in range(3)]
        km = np.concatenate([C.key_material(k.cipher, k.mac, k.etm, k.key, k.mac_key) for k in keys])
        km["etm"][2] = 2
        fn, want = lib.tlsrec_keytab_load_cbc, M.ERR_SSL_BAD_INPUT_DATA
    dev = torch.from_numpy(km.view(np.uint8).copy()).to(DEV) if on_device else None
    torch.cuda.synchronize()
    assert fn(kt.handle, 0, 3, dev.data_ptr() if on_device else km.ctypes.data, int(on_device), None) == want
    assert [_slot_cipher(kt, s) for s in range(4)] == [0, 0, 0, 0]
    assert _has_cbc(kt) == 0
    # and the device agrees: a record naming one of the slots gets the unusable-slot result
    batch = B.Batch([None] * 3, B.plaintext_records([None] * 3, [64, 64, 64], seed=5))
    out, res = batch.run_gpu(False, kt=kt)
    assert [int(r["status"]) for r in res] == [M.ERR_SSL_BAD_INPUT_DATA] * 3
    kt.close()


def test_engine_slot_allocate_free_allocate():
    """a transform's slots go back to the engine when it closes and the next transform gets the same numbers, under
    another key: one record through each, both the oracle's"""
    got = []
    for turn in range(2):
        key, iv = prng_bytes(90 + turn, 32), prng_bytes(95 + turn, 16)
        t = M.Transform(M.VERSION_TLS1_3, M.CIPHER_AES_256_GCM, key, key, iv, iv)
        ot = O.Transform(M.VERSION_TLS1_3, M.CIPHER_AES_256_GCM, key, key, iv, iv)
        try:
            got.append((int(t._t.slot_enc), int(t._t.slot_dec)))
            pt = prng_bytes(99 + turn, 64)
            ctr = (7 + turn).to_bytes(8, "big")
            rec = M.Record(ctr=ctr, type=23, ver=b"\x03\x03", buf=bytearray(pt) + bytearray(64), data_offset=0,
                           data_len=64)
            orec = O.Record(ctr=ctr, type=23, ver=b"\x03\x03", buf=bytearray(pt) + bytearray(64), data_offset=0,
                            data_len=64)
            assert t.encrypt_buf(rec) == 0 and ot.encrypt_buf(orec) == 0
            assert bytes(rec.buf) == bytes(orec.buf)
            assert (rec.data_offset, rec.data_len, rec.type) == (orec.data_offset, orec.data_len, orec.type)
            assert t.decrypt_buf(rec) == 0 and rec.data() == pt
        finally:
            t.close()
    assert got[0][0] >= 0 and got[0][1] >= 0 and got[0][0] != got[0][1]
    assert got[1] == got[0], "the freed slots were not the next ones allocated"
