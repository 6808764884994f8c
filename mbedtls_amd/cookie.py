"""DTLS cookies on the GPU (tlsrec_cookie_* / tlsrec_dtls_check_clihlo_cookies):
mbedtls_ssl_cookie_write / mbedtls_ssl_cookie_check of library/ssl_cookie.c and
mbedtls_ssl_check_dtls_clihlo_cookie (library/ssl_msg.c) for a batch of
first-flight datagrams in device memory, all under one secret."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _abi
from .batch import _ptr, _stream

COOKIE_ITEM, CLIHLO, CLIHLO_RES = _abi.COOKIE_ITEM, _abi.CLIHLO, _abi.CLIHLO_RES
COOKIE_LEN, HVR_LEN, TIMEOUT = _abi.COOKIE_LEN, _abi.DTLS_HVR_LEN, _abi.COOKIE_TIMEOUT


class CookieContext:
    """tlsrec_cookie_ctx: the HMAC midstates of one secret on the current HIP
    device and the timeout.  key None: 32 random bytes drawn by the library."""

    def __init__(self, key: bytes | None = None, timeout: int = TIMEOUT):
        self._lib = _abi.load()
        if key is not None and len(key) != 32:
            raise ValueError("a cookie key is 32 bytes")
        h = ctypes.c_void_p()
        r = self._lib.tlsrec_cookie_setup(ctypes.byref(h), key, timeout)
        if r != 0:
            raise RuntimeError(f"tlsrec_cookie_setup failed: {r:#x}")
        self.handle = h

    def set_timeout(self, delay: int):
        self._lib.tlsrec_cookie_set_timeout(self.handle, delay)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.tlsrec_cookie_free(self.handle)
            self.handle = None

    __del__ = close

    def write(self, cli_id: bytes, space: int = COOKIE_LEN):
        """tlsrec_cookie_write into `space` bytes: (status, cookie bytes written, how far *p moved)"""
        buf = ctypes.create_string_buffer(max(space, 1))
        start = ctypes.addressof(buf)
        p = ctypes.c_void_p(start)
        r = self._lib.tlsrec_cookie_write(self.handle, ctypes.byref(p), start + space, bytes(cli_id), len(cli_id))
        moved = (p.value or 0) - start
        return r, buf.raw[:moved], moved

    def check(self, cookie: bytes, cli_id: bytes) -> int:
        return self._lib.tlsrec_cookie_check(self.handle, bytes(cookie), len(cookie), bytes(cli_id), len(cli_id))


def _items(items, like):
    if isinstance(items, np.ndarray):
        import torch
        items = torch.from_numpy(np.ascontiguousarray(items).view(np.uint8).reshape(-1).copy()).to(like.device)
    return items


def _run(fn, ctx: CookieContext, now: int, items, n: int, arenas, res, stream):
    items = _items(items, res)
    r = getattr(_abi.load(), fn)(ctx.handle, now, _ptr(items), n, *[_ptr(a) for a in arenas], _ptr(res),
                                 _stream(stream))
    if r != 0:
        raise RuntimeError(f"{fn} failed: {r}")


def batch_write(ctx, now, items, n, id_arena, cookie_arena, status, stream=None):
    """items: COOKIE_ITEM array (numpy, or its bytes on the device); status: int32 device tensor of n"""
    _run("tlsrec_cookie_batch_write", ctx, now, items, n, (id_arena, cookie_arena), status, stream)


def batch_check(ctx, now, items, n, id_arena, cookie_arena, status, stream=None):
    _run("tlsrec_cookie_batch_check", ctx, now, items, n, (id_arena, cookie_arena), status, stream)


def check_clihlo(ctx, now, hellos, n, arena, id_arena, out_arena, res, stream=None):
    """hellos: CLIHLO array; res: device tensor holding n CLIHLO_RES (8 bytes each)"""
    _run("tlsrec_dtls_check_clihlo_cookies", ctx, now, hellos, n, (arena, id_arena, out_arena), res, stream)
