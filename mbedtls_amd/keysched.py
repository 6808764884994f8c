"""TLS 1.3 key schedule on the GPU (library/ssl_tls13_keys.c), through the
C ABI of include/tlsrec.h.  Same arguments, outputs and error codes as the
reference functions; every hash / HMAC / HKDF step runs in a HIP kernel.

    mbedtls_ssl_tls13_hkdf_expand_label  (:138)  -> hkdf_expand_label
    mbedtls_ssl_tls13_derive_secret      (:293)  -> derive_secret
    mbedtls_ssl_tls13_evolve_secret      (:332)  -> evolve_secret
    mbedtls_ssl_tls13_make_traffic_keys  (:262)  -> make_traffic_keys
    mbedtls_ssl_tls13_exporter           (:1828) -> exporter
    KeyUpdate, "traffic upd" (ssl_tls13_keys.h:16, RFC 8446 7.2) -> update_traffic_secret
    batch: secrets in HBM -> key-table slots       -> keytab_derive
"""
from __future__ import annotations

import ctypes

from . import _abi
from .batch import KeyTable, _ptr, _stream

ALG_SHA_256 = _abi.ALG_SHA_256
ALG_SHA_384 = _abi.ALG_SHA_384
CONTEXT_UNHASHED = _abi.TLS13_CONTEXT_UNHASHED
CONTEXT_HASHED = _abi.TLS13_CONTEXT_HASHED
HASH_LEN = {ALG_SHA_256: 32, ALG_SHA_384: 48}


class KeyScheduleError(RuntimeError):
    def __init__(self, fn, code):
        super().__init__(f"{fn} failed: {code}")
        self.code = code


def _chk(fn, r):
    if r != 0:
        raise KeyScheduleError(fn, r)


def _b(x):
    return None if x is None else bytes(x)


def hkdf_expand_label(hash_alg: int, secret: bytes, label: bytes, ctx: bytes, n: int) -> bytes:
    out = ctypes.create_string_buffer(max(1, n))
    _chk("tlsrec_tls13_hkdf_expand_label", _abi.load().tlsrec_tls13_hkdf_expand_label(
        hash_alg, _b(secret), len(secret), _b(label), len(label), _b(ctx), len(ctx), out, n))
    return out.raw[:n]


def derive_secret(hash_alg: int, secret: bytes, label: bytes, ctx: bytes, ctx_hashed: int, n: int) -> bytes:
    out = ctypes.create_string_buffer(max(1, n))
    _chk("tlsrec_tls13_derive_secret", _abi.load().tlsrec_tls13_derive_secret(
        hash_alg, _b(secret), len(secret), _b(label), len(label), _b(ctx), len(ctx), ctx_hashed, out, n))
    return out.raw[:n]


def evolve_secret(hash_alg: int, secret_old: bytes | None, inp: bytes | None) -> bytes:
    out = ctypes.create_string_buffer(64)
    _chk("tlsrec_tls13_evolve_secret", _abi.load().tlsrec_tls13_evolve_secret(
        hash_alg, _b(secret_old) or None, _b(inp) or None, len(inp or b""), out))
    return out.raw[:HASH_LEN[hash_alg]]


def make_traffic_keys(hash_alg: int, client_secret: bytes, server_secret: bytes, key_len: int, iv_len: int):
    ks = _abi.CKeySet()
    _chk("tlsrec_tls13_make_traffic_keys", _abi.load().tlsrec_tls13_make_traffic_keys(
        hash_alg, _b(client_secret), _b(server_secret), len(client_secret), key_len, iv_len, ctypes.byref(ks)))
    return (bytes(ks.client_write_key[:key_len]), bytes(ks.client_write_iv[:iv_len]),
            bytes(ks.server_write_key[:key_len]), bytes(ks.server_write_iv[:iv_len]))


def exporter(hash_alg: int, secret: bytes, label: bytes, context: bytes, n: int) -> bytes:
    out = ctypes.create_string_buffer(max(1, n))
    _chk("tlsrec_tls13_exporter", _abi.load().tlsrec_tls13_exporter(
        hash_alg, _b(secret), len(secret), _b(label), len(label), _b(context), len(context), out, n))
    return out.raw[:n]


def update_traffic_secret(hash_alg: int, secret: bytes) -> bytes:
    out = ctypes.create_string_buffer(64)
    _chk("tlsrec_tls13_update_traffic_secret",
         _abi.load().tlsrec_tls13_update_traffic_secret(hash_alg, _b(secret), out))
    return out.raw[:HASH_LEN[hash_alg]]


def keytab_derive(kt: KeyTable, first: int, count: int, cipher: int, secrets, key_update: bool = False,
                  stream=None) -> None:
    """`secrets`: device buffer (uint8 tensor) of count x 48 bytes
    (tlsrec_tls13_secret); updated in place when key_update."""
    _chk("tlsrec_tls13_keytab_derive", _abi.load().tlsrec_tls13_keytab_derive(
        kt.handle, first, count, cipher, _ptr(secrets), int(bool(key_update)), _stream(stream)))


# ---- the rest of the ladder (RFC 8446 7.1) ---------------------------------------
#    mbedtls_ssl_tls13_derive_early_secrets            (:421) -> derive_early_secrets
#    mbedtls_ssl_tls13_derive_handshake_secrets        (:479) -> derive_handshake_secrets
#    mbedtls_ssl_tls13_derive_application_secrets      (:545) -> derive_application_secrets
#    mbedtls_ssl_tls13_derive_resumption_master_secret (:621) -> derive_resumption_master_secret
#    ssl_tls13_calc_finished_core                      (:697) -> calc_finished
#    mbedtls_ssl_tls13_create_psk_binder               (:832) -> create_psk_binder
#    batches: keytab_derive_handshake, keytab_derive_application, batch_verify_data, batch_derive_secret
PSK_EXTERNAL = _abi.TLS13_PSK_EXTERNAL
PSK_RESUMPTION = _abi.TLS13_PSK_RESUMPTION
SECRET_BYTES = ctypes.sizeof(_abi.CTls13Secret)      # 48
HS_CONN_BYTES = ctypes.sizeof(_abi.CTls13HsConn)     # 176: psk[48] || shared[80] || transcript[48]


def _helper(name, struct, fields, hash_alg, secret, transcript):
    out = struct()
    _chk(name, getattr(_abi.load(), name)(hash_alg, _b(secret), _b(transcript), len(transcript), ctypes.byref(out)))
    n = HASH_LEN[hash_alg]
    return tuple(bytes(getattr(out, f)[:n]) for f in fields)


def derive_early_secrets(hash_alg: int, early_secret: bytes, transcript: bytes):
    """(client_early_traffic_secret, early_exporter_master_secret)"""
    return _helper("tlsrec_tls13_derive_early_secrets", _abi.CTls13EarlySecrets,
                   ("client_early_traffic_secret", "early_exporter_master_secret"), hash_alg, early_secret, transcript)


def derive_handshake_secrets(hash_alg: int, handshake_secret: bytes, transcript: bytes):
    """(client_handshake_traffic_secret, server_handshake_traffic_secret)"""
    return _helper("tlsrec_tls13_derive_handshake_secrets", _abi.CTls13HandshakeSecrets,
                   ("client_handshake_traffic_secret", "server_handshake_traffic_secret"), hash_alg,
                   handshake_secret, transcript)


def derive_application_secrets(hash_alg: int, master_secret: bytes, transcript: bytes):
    """(client_application_traffic_secret_0, server_application_traffic_secret_0, exporter_master_secret)"""
    return _helper("tlsrec_tls13_derive_application_secrets", _abi.CTls13ApplicationSecrets,
                   ("client_application_traffic_secret_N", "server_application_traffic_secret_N",
                    "exporter_master_secret"), hash_alg, master_secret, transcript)


def derive_resumption_master_secret(hash_alg: int, master_secret: bytes, transcript: bytes) -> bytes:
    return _helper("tlsrec_tls13_derive_resumption_master_secret", _abi.CTls13ApplicationSecrets,
                   ("resumption_master_secret",), hash_alg, master_secret, transcript)[0]


def calc_finished(hash_alg: int, base_secret: bytes, transcript: bytes) -> bytes:
    """verify_data of a Finished message under `base_secret` (a handshake traffic secret)"""
    out, n = ctypes.create_string_buffer(64), ctypes.c_size_t(0)
    _chk("tlsrec_tls13_calc_finished", _abi.load().tlsrec_tls13_calc_finished(
        hash_alg, _b(base_secret), _b(transcript), out, ctypes.byref(n)))
    return out.raw[:n.value]


def create_psk_binder(hash_alg: int, psk: bytes, psk_type: int, transcript: bytes) -> bytes:
    out = ctypes.create_string_buffer(64)
    _chk("tlsrec_tls13_create_psk_binder", _abi.load().tlsrec_tls13_create_psk_binder(
        hash_alg, _b(psk), len(psk), psk_type, _b(transcript), out))
    return out.raw[:HASH_LEN[hash_alg]]


def _h(kt):
    return kt.handle if kt is not None else None


def keytab_derive_handshake(kt: KeyTable, first: int, count: int, cipher: int, psk_len: int, shared_len: int, conns,
                            hs_traffic, finished_keys, master, stream=None) -> None:
    """`conns`: device buffer of count x 176 bytes (tlsrec_tls13_hs_conn), only
    read.  Outputs, device buffers of 48-byte elements: hs_traffic and
    finished_keys (or None) 2 x count in slot order, master count.  Connection
    i's client_write keys land in slot first + 2*i, server_write in first + 2*i + 1
    (mbedtls_amd.tls12.tls12_slots gives an endpoint's pair)."""
    _chk("tlsrec_tls13_keytab_derive_handshake", _abi.load().tlsrec_tls13_keytab_derive_handshake(
        _h(kt), first, count, cipher, psk_len, shared_len, _ptr(conns), _ptr(hs_traffic), _ptr(finished_keys),
        _ptr(master), _stream(stream)))


def keytab_derive_application(kt: KeyTable, first: int, count: int, cipher: int, master, transcripts, app_traffic,
                              exporter, stream=None) -> None:
    """`master`, `transcripts` (Hash(ClientHello..server Finished)): count x 48
    bytes on the device; app_traffic 2 x count in slot order (what keytab_derive
    takes for a KeyUpdate), exporter count or None."""
    _chk("tlsrec_tls13_keytab_derive_application", _abi.load().tlsrec_tls13_keytab_derive_application(
        _h(kt), first, count, cipher, _ptr(master), _ptr(transcripts), _ptr(app_traffic), _ptr(exporter),
        _stream(stream)))


def batch_verify_data(hash_alg: int, finished_keys, transcripts, out, count: int, stream=None) -> None:
    """out[i] = HMAC(finished_keys[i], transcripts[i]); device buffers of 48-byte elements"""
    _chk("tlsrec_tls13_batch_verify_data", _abi.load().tlsrec_tls13_batch_verify_data(
        hash_alg, _ptr(finished_keys), _ptr(transcripts), _ptr(out), count, _stream(stream)))


def batch_derive_secret(hash_alg: int, label: bytes, secrets, transcripts, out, count: int, stream=None) -> None:
    """out[i] = Derive-Secret(secrets[i], label, hashed context transcripts[i]); label of at most 12 bytes"""
    _chk("tlsrec_tls13_batch_derive_secret", _abi.load().tlsrec_tls13_batch_derive_secret(
        hash_alg, _b(label), len(label), _ptr(secrets), _ptr(transcripts), _ptr(out), count, _stream(stream)))


def batch_exporter(hash_alg: int, secrets, label: bytes, contexts, context_len: int, context_stride: int, out,
                   out_len: int, out_stride: int, count: int, stream=None) -> None:
    """mbedtls_ssl_tls13_exporter (:1828) for count connections: out[i * out_stride .. + out_len)
    from secrets[i] (count x 48 bytes on the device: the `exporter` of keytab_derive_application
    or the `early_exporter` of keytab_derive_early).  `label`: host bytes, at most 249.
    `contexts`: device bytes, context_len (at most 255) at i * context_stride, stride 0 = one
    shared context, None with context_len 0 = no context."""
    _chk("tlsrec_tls13_batch_exporter", _abi.load().tlsrec_tls13_batch_exporter(
        hash_alg, _ptr(secrets), _b(label), len(label), _ptr(contexts), context_len, context_stride, _ptr(out),
        out_len, out_stride, count, _stream(stream)))


# ---- a resumed handshake in batches ------------------------------------------------
#    ssl_tls13_offered_psks_check_binder_match (ssl_tls13_server.c:404)  -> batch_psk_binder
#    ssl_tls13_generate_early_key (:1086) + compute_early_transform (:1184) -> keytab_derive_early
#    the "resumption" Expand-Label (ssl_tls13_server.c:3219)             -> batch_ticket_psk
PSK_CONN_BYTES = ctypes.sizeof(_abi.CTls13PskConn)   # 144: psk[48] || binder_transcript[48] || hello_transcript[48]
TICKET_NONCE_BYTES = 32                              # MBEDTLS_SSL_TLS1_3_TICKET_NONCE_LENGTH


def batch_psk_binder(hash_alg: int, psk_len: int, psk_type: int, conns, offered, binders, match, count: int,
                     stream=None) -> None:
    """`conns`: device buffer of count x 144 bytes (tlsrec_tls13_psk_conn), only
    read.  binders (or None): count x 48 bytes.  offered (count x 48 bytes) and
    match (count x uint32: 1 where the first Hash.length bytes of offered[i] are
    the binder) go together; a client computing its own binders passes None, None."""
    _chk("tlsrec_tls13_batch_psk_binder", _abi.load().tlsrec_tls13_batch_psk_binder(
        hash_alg, psk_len, psk_type, _ptr(conns), _ptr(offered), _ptr(binders), _ptr(match), count, _stream(stream)))


def keytab_derive_early(kt: KeyTable, first: int, count: int, cipher: int, psk_len: int, psk_type: int, conns, offered,
                        binders, match, early_traffic, early_exporter, stream=None) -> None:
    """batch_psk_binder and, in the same pass, c e traffic -> early_traffic, e exp
    master -> early_exporter (or None), both count x 48 bytes, and the key / iv of
    c e traffic into slot first + i (client_write).  The slot is loaded whether
    or not the binder matched: where match[i] == 0 the connection is dropped and
    slot first + i must not be used."""
    _chk("tlsrec_tls13_keytab_derive_early", _abi.load().tlsrec_tls13_keytab_derive_early(
        _h(kt), first, count, cipher, psk_len, psk_type, _ptr(conns), _ptr(offered), _ptr(binders), _ptr(match),
        _ptr(early_traffic), _ptr(early_exporter), _stream(stream)))


def batch_ticket_psk(hash_alg: int, nonce_len: int, res_master, nonces, psk, count: int, stream=None) -> None:
    """psk[i] = HKDF-Expand-Label(res_master[i], "resumption", nonce i, Hash.length);
    `nonces`: count x 32 bytes on the device, the first nonce_len (0..32) of each used"""
    _chk("tlsrec_tls13_batch_ticket_psk", _abi.load().tlsrec_tls13_batch_ticket_psk(
        hash_alg, nonce_len, _ptr(res_master), _ptr(nonces), _ptr(psk), count, _stream(stream)))
