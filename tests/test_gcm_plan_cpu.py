"""The launch shapes of a batch (csrc/tlsrec_plan.h gcm_plan / chacha_plan,
host functions: no GPU needed) against tests/golden/gcm_plan.json -- the
shapes the batch path logged on an MI355X before the rule moved into those
functions (tests/golden/make_gcm_plan.py), one row on each side of every
threshold -- and the invariants a launch relies on."""
import json
import os

import pytest

from mbedtls_amd import _abi

KNOBS = ["TLSREC_GCM_WP", "TLSREC_GCM_G5", "TLSREC_GCM_TREEMUL", "TLSREC_GCM_HBUILD", "TLSREC_GCM_PAIR",
         "TLSREC_GROUPED", "TLSREC_GCM_SRECS", "TLSREC_GCM_PAIR_L", "TLSREC_GCM_PAIR_SMALL_MAX",
         "TLSREC_GCM_PAIR_SMALL_MIN", "TLSREC_GCM_PAIR_BIG_MAX", "TLSREC_GCM_LANES"]
NR = {_abi.CIPHER_AES_128_GCM: 10, _abi.CIPHER_AES_192_GCM: 12, _abi.CIPHER_AES_256_GCM: 14}
with open(os.path.join(os.path.dirname(__file__), "golden", "gcm_plan.json")) as _f:
    ROWS = json.load(_f)


def _plan_in(row):
    """a recorded row as GcmPlanIn fields, by batch()'s own few lines: which
    batches keep identity order, and the TLSREC_GCM_LANES fallback"""
    env = row["env"]
    grouped = row["path"] == "grouped" and env.get("TLSREC_GROUPED") != "0"
    identity = row["nkeys"] == 1 or row["n"] == 1 or grouped
    assert int(not identity) == row["bucket"], row          # the recorded batch took the order restated here
    return dict(n=row["n"], nloaded=row["nkeys"], cu=row["cu"], avg_bytes=0 if row["path"] == "lanes" else row["avg_bytes"],
                lanes=row["lanes"] or int(env.get("TLSREC_GCM_LANES", 0)), nr=NR[row["cipher"]], has_cid=row["cid"],
                coalesced=0, keyrun=int(not identity or grouped))


@pytest.fixture
def plan_of(monkeypatch):
    """row -> its plan, computed under the row's switches and no others"""
    def plan(row):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in row["env"].items():
            monkeypatch.setenv(k, v)
        if row["cipher"] == _abi.CIPHER_CHACHA20_POLY1305:
            return _abi.chacha_plan(row["n"], row["cu"], row["lanes"], row["cid"])
        return _abi.gcm_plan(**_plan_in(row))
    return plan


def test_golden_file_covers_the_rule():
    assert len(ROWS) >= 100
    envs = {k for r in ROWS for k in r["env"]}
    assert envs >= {"TLSREC_GCM_WP", "TLSREC_GCM_PAIR", "TLSREC_GCM_PAIR_L", "TLSREC_GCM_TREEMUL", "TLSREC_GCM_HBUILD",
                    "TLSREC_GROUPED", "TLSREC_GCM_G5", "TLSREC_GCM_PAIR_SMALL_MIN", "TLSREC_GCM_PAIR_SMALL_MAX",
                    "TLSREC_GCM_PAIR_BIG_MAX", "TLSREC_GCM_LANES"}
    assert {r["cipher"] for r in ROWS} == set(NR) | {_abi.CIPHER_CHACHA20_POLY1305}
    assert {r.get("code") for r in ROWS} == {16, -8, -16, -32, None}
    assert {r["L"] for r in ROWS if "code" in r} == {2, 4, 8, 16, 32, 64}
    assert any(r["cid"] for r in ROWS) and {r["path"] for r in ROWS} == {"lanes", "sized", "grouped"}


def test_plans_match_the_recorded_launches(plan_of):
    bad = []
    for i, row in enumerate(ROWS):
        p = plan_of(row)
        got = (p.L,) if row["cipher"] == _abi.CIPHER_CHACHA20_POLY1305 else (p.L, p.code, p.tm)
        want = (row["L"],) if len(got) == 1 else (row["L"], row["code"], row["tm"])
        if got != want:
            bad.append((i, row, got))
    assert not bad, bad[:5]


def test_plans_cover_the_batch(plan_of):
    """rpw in whole rounds of 64 / L records, at most 64; the grid covers n and
    has no idle workgroup"""
    for row in ROWS:
        p = plan_of(row)
        waves = 4 if row["cipher"] == _abi.CIPHER_CHACHA20_POLY1305 else p.waves
        assert p.rpw % (64 // p.L) == 0 and 1 <= p.rpw <= 64, (row, p.rpw)
        assert p.grid * waves * p.rpw >= row["n"] > (p.grid - 1) * waves * p.rpw, (row, p.grid, p.rpw)
        if waves != 4:
            assert waves == {-32: 16, -8: 8, -16: 16}.get(p.code, p.code) and p.g5 == int(
                row["env"].get("TLSREC_GCM_G5") != "0")


def _default_knobs():
    """the switches' values in an empty environment, as csrc/tlsrec_plan.h documents them"""
    return _abi.GcmKnobs(waves=16, wp=-1, g5=1, treemul=-1, hbuild=1, pair=1, grouped=1, srecs=0, pair_l=0,
                         pair_small_min=12, pair_small_max=256, pair_big_max=40, lanes=0)


def test_explicit_knobs_equal_the_empty_environment(plan_of):
    for row in ROWS:
        if row["env"] or row["cipher"] == _abi.CIPHER_CHACHA20_POLY1305:
            continue
        p, q = plan_of(row), _abi.gcm_plan(_default_knobs(), **_plan_in(row))
        assert [getattr(p, f) for f, _ in p._fields_] == [getattr(q, f) for f, _ in q._fields_], row


def test_coalesced_batch_is_a_wave_per_record():
    """records gathered from concurrent single-record calls (not reachable as
    one deterministic batch on the device): 64 lanes, 8-wave wave passes, the
    lane tree from the key's tables, one record per wave"""
    for nr in (10, 14):
        p = _abi.gcm_plan(_default_knobs(), n=7, nloaded=5, cu=256, avg_bytes=0, lanes=0, nr=nr, has_cid=0, coalesced=1,
                          keyrun=0)
        assert (p.L, p.code, p.tm, p.rpw, p.grid) == (64, -8, 0, 1, 1)
    p = _abi.gcm_plan(_default_knobs(), n=1, nloaded=5, cu=256, avg_bytes=0, lanes=0, nr=14, has_cid=0, coalesced=1,
                      keyrun=0)
    assert (p.L, p.code, p.tm) == (64, 16, 0)            # one record: the key pass, still from the tables


# tests/test_send_inplace_gpu.py _shape_cases(256): the in-place send path's batches (grouped, the fragment size
# as the hint) as plan inputs -- (cipher, keys, records, hint) -> the launch-log entry the GPU test expects
G128, G192, G256 = _abi.CIPHER_AES_128_GCM, _abi.CIPHER_AES_192_GCM, _abi.CIPHER_AES_256_GCM
CU = 256
SHAPES = {
    "gcm-one-key-8": (G128, 1, 64 * CU * 2, 48, (8, 16, 1)),
    "gcm-one-key-4": (G256, 1, 64 * CU * 4, 48, (4, 16, 1)),
    "gcm-wave-16": (G256, CU * 8, CU * 8 * 4, 200, (16, -8, 9)),
    "gcm-wave-64": (G128, 48, 48 * 2, 300, (64, -8, 9)),
    "gcm-pair-8": (G256, CU * 8, CU * 8 * 16, 100, (8, -32, 31)),
    "gcm-pair-4": (G128, CU * 8, CU * 8 * 32, 100, (4, -32, 31)),
    "gcm-pair-2": (G256, CU * 8, CU * 8 * 64, 100, (2, -32, 31)),
    "gcm-pair-big-32": (G128, CU * 8, CU * 8 * 4, 4100, (32, -32, 31)),
    "gcm-pair-big-16": (G256, CU * 4, CU * 4 * 16, 4100, (16, -32, 31)),
    "gcm192-key-pass-64": (G192, CU * 8, CU * 8 * 4, 200, (64, 16, 1)),
    "gcm192-key-pass-16": (G192, CU * 8, CU * 8 * 64, 100, (16, 16, 1)),
    "chacha-8": (None, 64, 64 * CU, 64, (8,)),
    "chacha-4": (None, 64, 64 * CU * 2, 64, (4,)),
    "chacha-2": (None, 64, 64 * CU * 4, 64, (2,)),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_send_path_shapes(case):
    cipher, nkeys, n, hint, want = SHAPES[case]
    if cipher is None:
        assert (_abi.chacha_plan(n, CU, 0, 0).L,) == want
        return
    p = _abi.gcm_plan(_default_knobs(), n=n, nloaded=nkeys, cu=CU, avg_bytes=hint, lanes=0, nr=NR[cipher], has_cid=0,
                      coalesced=0, keyrun=1)
    assert (p.L, p.code, p.tm) == want
