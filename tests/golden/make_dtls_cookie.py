#!/usr/bin/env python3
"""Transcribe the reference's ClientHello cookie-parsing test vectors into
tests/golden/dtls_cookie.json (data only: inputs and expected outputs).

Run where a checkout of the reference (Mbed TLS 4.1.0) is at hand:
    python tests/golden/make_dtls_cookie.py <reference tree>

Source: tests/suites/test_suite_ssl.data:3329-3345 of the reference, the cases
of cookie_parsing (test_suite_ssl.function:3700-3728): the datagram goes
through mbedtls_ssl_check_dtls_clihlo_cookie with the context's default cookie
callbacks (both fail: no cookie context is set up) and an output buffer of
MBEDTLS_SSL_OUT_CONTENT_LEN bytes, and must return `ret`.
"""
from __future__ import annotations

import json
import os
import re
import sys

REF = "tests/suites/test_suite_ssl.data"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dtls_cookie.json")
CODES = {"MBEDTLS_ERR_SSL_INTERNAL_ERROR": -0x6C00, "MBEDTLS_ERR_SSL_DECODE_ERROR": -0x7300}


def main():
    lines = open(os.path.join(sys.argv[1], REF), errors="replace").read().splitlines()
    cases = []
    for i, line in enumerate(lines):
        m = re.match(r'^cookie_parsing:"([0-9a-fA-F]*)":(MBEDTLS_ERR_SSL_[A-Z_]+)$', line)
        if not m:
            continue
        cases.append({"name": lines[i - 1], "line": i + 1, "datagram": m.group(1).lower(), "ret_name": m.group(2),
                      "ret": CODES[m.group(2)]})
    assert len(cases) == 6, len(cases)
    json.dump({"source": "tests/suites/test_suite_ssl.data (cookie_parsing)", "cases": cases},
              open(OUT, "w"), indent=1)
    print(OUT, len(cases))


if __name__ == "__main__":
    main()
