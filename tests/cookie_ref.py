"""The DTLS cookie functions restated over hmac / hashlib: the checker of the
cookie tests.

mbedtls_ssl_cookie_write / mbedtls_ssl_cookie_check (library/ssl_cookie.c
:117-179, :184-250) and mbedtls_ssl_check_dtls_clihlo_cookie (library/ssl_msg.c
:3322-3454), statement by statement, with the time passed in.  Every function
returns (status, bytes written).
"""
from __future__ import annotations

import hashlib
import hmac
import struct

BAD_INPUT_DATA, BUFFER_TOO_SMALL = -135, -138
INVALID_MAC, INTERNAL_ERROR = -0x7180, -0x6C00
DECODE_ERROR, HELLO_VERIFY_REQUIRED = -0x7300, -0x6A80
COOKIE_LEN, HMAC_LEN, HVR_LEN = 32, 28, 60
M64 = (1 << 64) - 1


def _mac(key: bytes, stamp: bytes, cli_id: bytes) -> bytes:
    return hmac.new(key, stamp + cli_id, hashlib.sha256).digest()[:HMAC_LEN]


def cookie_write(key: bytes, now: int, cli_id: bytes, space: int):
    """ssl_cookie.c:117-179 into `space` bytes (end - *p); cli_id None / longer than the ABI's 255: BAD_INPUT_DATA"""
    if cli_id is None or len(cli_id) > 255:
        return BAD_INPUT_DATA, b""
    if space < COOKIE_LEN:                                   # MBEDTLS_SSL_CHK_BUF_PTR, :132
        return BUFFER_TOO_SMALL, b""
    stamp = struct.pack(">I", now & 0xffffffff)              # MBEDTLS_PUT_UINT32_BE(t), :140
    return 0, stamp + _mac(key, stamp, cli_id)


def cookie_check(key: bytes, timeout: int, now: int, cookie: bytes, cli_id: bytes):
    """ssl_cookie.c:184-250"""
    if cli_id is None or len(cli_id) > 255:
        return BAD_INPUT_DATA, b""
    if len(cookie) != COOKIE_LEN:                            # :198-200
        return -1, b""
    if not hmac.compare_digest(_mac(key, cookie[:4], cli_id), cookie[4:]):
        return INVALID_MAC, b""                              # PSA_ERROR_INVALID_SIGNATURE, ssl_tls.c:2157-2166
    cookie_time = struct.unpack(">I", cookie[:4])[0]
    if timeout != 0 and ((now - cookie_time) & M64) > timeout:     # unsigned long, :239
        return -1, b""
    return 0, b""


def check_clihlo(key: bytes, timeout: int, now: int, cli_id: bytes, dgram: bytes, out_cap: int):
    """ssl_msg.c:3322-3454; the bytes are the HelloVerifyRequest (empty unless
    HELLO_VERIFY_REQUIRED: what the reference leaves in obuf on the other
    paths is no output of it)"""
    n = len(dgram)
    if n < 61:
        return DECODE_ERROR, b""
    epoch = (dgram[3] << 8) | dgram[4]
    fragment_offset = (dgram[19] << 16) | (dgram[20] << 8) | dgram[21]
    if dgram[0] != 22 or epoch != 0 or fragment_offset != 0:
        return DECODE_ERROR, b""
    sid_len = dgram[59]
    if 59 + 1 + sid_len + 1 > n:
        return DECODE_ERROR, b""
    cookie_len = dgram[60 + sid_len]
    if 59 + 1 + sid_len + 1 + cookie_len > n:
        return DECODE_ERROR, b""
    if cookie_check(key, timeout, now, dgram[61 + sid_len:61 + sid_len + cookie_len], cli_id)[0] == 0:
        return 0, b""
    if out_cap < 28:
        return BUFFER_TOO_SMALL, b""
    obuf = bytearray(dgram[:25]) + bytearray(3)
    obuf[13] = 3                                             # MBEDTLS_SSL_HS_HELLO_VERIFY_REQUEST
    obuf[25], obuf[26] = 0xfe, 0xff
    st, cookie = cookie_write(key, now, cli_id, out_cap - 28)
    if st != 0:
        return INTERNAL_ERROR, b""
    obuf += cookie
    olen = len(obuf)
    obuf[27] = olen - 28
    obuf[14:17] = obuf[22:25] = (olen - 25).to_bytes(3, "big")
    obuf[11:13] = (olen - 13).to_bytes(2, "big")
    return HELLO_VERIFY_REQUIRED, bytes(obuf)
