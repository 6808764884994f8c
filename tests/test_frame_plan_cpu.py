"""The receive framing plans (csrc/tlsrec_plan.h stream_rx_plan / dtls_rx_plan,
host functions: no GPU needed) on both sides of every threshold.  They restate
what the GPU tests read from the launch log: tests/test_dtls_stash_gpu.py
(_expected_s, DTLS_GUARD, the STREAM_RX_FRAME tuple of
test_stream_max_records_guard) and tests/test_stream_gpu.py."""
import itertools

import pytest

from mbedtls_amd import _abi

KNOBS = ["TLSREC_RX_GROUPWALK", "TLSREC_RX_FUSED_STREAM", "TLSREC_RX_RG", "TLSREC_RX_FUSED", "TLSREC_DTLS_STASH",
         "TLSREC_RX_PREFILL", "TLSREC_RX_MAILBOX", "TLSREC_STREAM_SRC"]
RX_TILE = 128          # PLAN_RX_TILE: connections of a one-pass stream tile, at every G
RX_THREADS = 256       # a count / emit workgroup: 256 / G connections
DG_TILE = 256          # connections of a DTLS tile


@pytest.fixture
def env(monkeypatch):
    """set exactly these switches (None: unset), every other one unset"""
    def set_env(**kv):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kv.items():
            if v is not None:
                monkeypatch.setenv("TLSREC_" + k, v)
    return set_env


def _fields(p):
    return [getattr(p, f) for f, _ in p._fields_]


def _default_knobs():
    """the switches' values in an empty environment, as csrc/tlsrec_plan.h documents them"""
    return _abi.FrameKnobs(groupwalk=1, fused_stream=0, rg=0, fused=1, stash=1, prefill=1, mailbox=1, stream_src=1)


def _ceil(a, b):
    return (a + b - 1) // b


# ---- DTLS -------------------------------------------------------------------------
def _expected_s(per, stash, fused):
    """tests/test_dtls_stash_gpu.py _expected_s"""
    if fused == "0":
        return -1
    return 0 if (stash == "0" or per > 16) else (16 if per > 4 else 4)


@pytest.mark.parametrize("nconns", [1, 256, 257])
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("stash", [None, "0"])
@pytest.mark.parametrize("per", [1, 4, 5, 16, 17])
def test_dtls_plan(per, stash, fused, nconns, env):
    env(DTLS_STASH=stash, RX_FUSED=fused)
    for ndgrams in {nconns * (per - 1) + 1, nconns * per}:          # both ends of ceil(ndgrams / nconns) == per
        assert _ceil(ndgrams, nconns) == per
        p = _abi.dtls_rx_plan(nconns, ndgrams)
        assert (p.fused, p.S) == (int(fused == "1"), _expected_s(per, stash, fused)), (nconns, ndgrams)
        assert p.tiles == _ceil(nconns, DG_TILE) and p.tiles * DG_TILE >= nconns > (p.tiles - 1) * DG_TILE


def test_dtls_guard_cases(env):
    """tests/test_dtls_stash_gpu.py DTLS_GUARD: 260 connections of `per` datagrams"""
    for per, fused, want_s in [(3, "1", 4), (6, "1", 16), (17, "1", 0), (6, "0", -1)]:
        env(RX_FUSED=fused)
        assert _abi.dtls_rx_plan(260, 260 * per).S == want_s


# ---- stream -----------------------------------------------------------------------
def _expected_g(per, rg, gw):
    if gw == "0":
        return 1
    if rg in ("4", "8", "16"):
        return int(rg)
    return 4 if per <= 4 else (8 if per <= 8 else 16)


@pytest.mark.parametrize("gw,fs", [(None, None), (None, "1"), ("0", None), ("0", "1")])
@pytest.mark.parametrize("rg", [None, "4", "8", "16", "5"])
@pytest.mark.parametrize("per", [1, 4, 5, 8, 9, 16, 100])
def test_stream_plan(per, rg, gw, fs, env):
    env(RX_RG=rg, RX_GROUPWALK=gw, RX_FUSED_STREAM=fs)
    for nstreams in (1, 127, 128, 129, 255, 256, 257, 515, 65536):
        for max_records in {nstreams * (per - 1) + 1, nstreams * per}:
            assert _ceil(max_records, nstreams) == per
            p = _abi.stream_rx_plan(nstreams, max_records)
            g = _expected_g(per, rg, gw)
            assert p.G == g, (nstreams, max_records)
            assert p.fused == int(fs == "1" and gw != "0")          # one pass only with the group walk: never at G = 1
            assert p.tile == RX_TILE and p.tiles * p.tile >= nstreams > (p.tiles - 1) * p.tile
            conns = RX_THREADS // g                                  # of a count / emit workgroup
            assert p.emit_grid * conns >= nstreams > (p.emit_grid - 1) * conns
            assert p.count_grid * conns >= nstreams + 1 > (p.count_grid - 1) * conns      # the scan's sentinel


def test_stream_log_tuples_of_the_gpu_legs(env):
    """tests/test_stream_gpu.py FRAMINGS (gw, fused, rg) -> the STREAM_RX_FRAME entry's (p0, p1)"""
    legs = {("1", "1", "16"): (1, 16), ("1", "0", "16"): (0, 16), ("1", "0", "8"): (0, 8), ("1", "0", "4"): (0, 4),
            ("0", "0", "16"): (0, 1)}
    for (gw, fused, rg), want in legs.items():
        env(RX_GROUPWALK=gw, RX_FUSED_STREAM=fused, RX_RG=rg)
        p = _abi.stream_rx_plan(300, 900)
        assert (p.fused, p.G) == want


def test_no_connections(env):
    env()
    assert _fields(_abi.stream_rx_plan(0, 0)) == [0, 16, RX_TILE, 0, 1, 0]
    assert _fields(_abi.dtls_rx_plan(0, 0)) == [1, 4, 0]


def test_explicit_knobs_equal_the_empty_environment(env):
    env()
    for n, m in itertools.product([1, 128, 129, 515, 70000], [0, 1, 515, 4 * 515, 8 * 515 + 1, 1 << 20]):
        assert _fields(_abi.stream_rx_plan(n, m)) == _fields(_abi.stream_rx_plan(n, m, _default_knobs())), (n, m)
        assert _fields(_abi.dtls_rx_plan(n, m)) == _fields(_abi.dtls_rx_plan(n, m, _default_knobs())), (n, m)


def test_knobs_are_read_from_the_environment(env):
    """every switch moves the plan it belongs to, and only as documented"""
    env(RX_FUSED="0")
    assert _abi.dtls_rx_plan(300, 1500).S == -1 and _abi.stream_rx_plan(300, 1500).fused == 0
    env(RX_FUSED_STREAM="1")
    assert _abi.stream_rx_plan(300, 1500).fused == 1 and _abi.dtls_rx_plan(300, 1500).S == 16
    k = _default_knobs()
    k.groupwalk, k.fused_stream, k.rg = 0, 1, 8
    p = _abi.stream_rx_plan(515, 515 * 3, k)
    assert (p.fused, p.G, p.count_grid, p.emit_grid) == (0, 1, 3, 3)
