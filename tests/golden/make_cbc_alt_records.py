"""Writes tests/golden/cbc_alt_records.json: 16 small ARIA-CBC / Camellia-CBC +
HMAC records (the four suites, both MAC orders, with and without a DTLS 1.2
connection ID) as tests/cbc_alt_ref.py seals them, plus what it makes of each
on decryption.  tests/test_cbc_alt_cpu.py pins the model to this file.

    python tests/golden/make_cbc_alt_records.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import cbc_alt_ref as A      # noqa: E402
from tests import cbc_ref as R          # noqa: E402
from tests.prng import prng_bytes       # noqa: E402


def cases():
    out = []
    n = 0
    for cipher, mac in A.SUITES:
        for etm in (0, 1):
            for cid in (b"", bytes(range(0x40, 0x47))):
                n += 1
                raw = prng_bytes(1900 + n, 80)
                key = R.Key(cipher, mac, etm, raw[:A.KEYLEN[cipher]], raw[32:32 + R.MACLEN[mac]], cid)
                length = [0, 1, 15, 16, 43, 64][n % 6]
                ver = b"\xfe\xfd" if cid or n % 3 == 0 else b"\x03\x03"
                ctr = prng_bytes(1300 + n, 8)
                buf = prng_bytes(1500 + n, 16 + length) + bytes(96)
                e = A.encrypt(key, buf, 16, length, ctr, 23, ver)
                assert e.status == 0
                d = A.decrypt(key, e.buf, e.data_offset, e.data_len, ctr, e.type, ver, cid)
                assert d.status == 0 and d.data_len == length and d.type == 23
                out.append({"cipher": cipher, "mac": mac, "etm": etm, "cid": cid.hex(), "key": key.key.hex(),
                            "mac_key": key.mac_key.hex(), "ver": ver.hex(), "ctr": ctr.hex(), "type": 23,
                            "plain": buf.hex(), "data_offset": 16, "data_len": length,
                            "sealed": e.buf.hex(), "sealed_offset": e.data_offset, "sealed_len": e.data_len,
                            "sealed_type": e.type, "opened_offset": d.data_offset})
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "cbc_alt_records.json"), "w") as f:
        json.dump(cases(), f, indent=0)
        f.write("\n")
