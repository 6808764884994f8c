"""Harness of the ARIA-CBC / Camellia-CBC tests: tests/cbclib.py's, with the
model of tests/cbc_alt_ref.py behind it.  Test-side only."""
from __future__ import annotations

from tests import cbc_alt_ref as A
from tests import cbclib as L
from tests import cbc_ref as R
from tests.prng import prng_bytes

# (cipher, mac, etm): the four suites in both MAC orders
ALT_KEYS = [(c, m, e) for c, m in A.SUITES for e in (0, 1)]
load_table, plain_rec = L.load_table, L.plain_rec


def make_key(seed, cipher, mac, etm, cid=b""):
    b = prng_bytes(seed, 80)
    return R.Key(cipher, mac, etm, b[:A.ALL_KEYLEN[cipher]], b[32:32 + R.MACLEN[mac]], cid)


def sealed_rec(*args, **kw):
    with A.as_model():
        return L.sealed_rec(*args, **kw)


class Run(L.Run):
    def expected(self, decrypt):
        with A.as_model():
            return super().expected(decrypt)
