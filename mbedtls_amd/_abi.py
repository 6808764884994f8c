"""ctypes binding of include/tlsrec.h (the C ABI of libtlsrec.so).

This is the same binding a maintainer would add to a Python caller of the
reference record path; it loads the in-tree HIP library
and raises if it is missing -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libtlsrec.so")

# ---- constants (include/tlsrec.h, values of include/mbedtls/ssl.h) ----------
ERR_SSL_BAD_INPUT_DATA = -135
ERR_SSL_BUFFER_TOO_SMALL = -138
ERR_SSL_ALLOC_FAILED = -141
ERR_SSL_FEATURE_UNAVAILABLE = -0x7080
ERR_SSL_INVALID_MAC = -0x7180
ERR_SSL_INVALID_RECORD = -0x7200
ERR_SSL_HW_ACCEL_FAILED = -0x7F80
ERR_SSL_INTERNAL_ERROR = -0x6C00
ERR_SSL_UNEXPECTED_CID = -0x6000
ERR_SSL_COUNTER_WRAPPING = -0x6B80
ERR_SSL_SESSION_TICKET_EXPIRED = -0x6D80
ERR_SSL_UNEXPECTED_RECORD = -0x6700
ERR_SSL_EARLY_MESSAGE = -0x6480
ERR_SSL_CONN_EOF = -0x7280
ERR_SSL_DECODE_ERROR = -0x7300
ERR_SSL_HELLO_VERIFY_REQUIRED = -0x6A80
COOKIE_TIMEOUT, COOKIE_LEN, DTLS_HVR_LEN = 60, 32, 60
DTLS_MAX_DATAGRAM = 16477
DTLS_OUT_BUFFER_LEN = 16477
DTLS_DROPPED, DTLS_NOT_REACHED = 1, 2
DTLS_ANTI_REPLAY, DTLS_IGNORE_UNEXPECTED_CID = 1, 2
MAX_IN_RECORD = 16421
OUT_BUF_SPACE = 16416
# a CBC slot's limits (the _ex framing calls with FRAME_CBC: the limit follows the slot's kind)
MAX_IN_RECORD_CBC, OUT_BUF_SPACE_CBC = 16709, 16704
DTLS_MAX_DATAGRAM_CBC = DTLS_OUT_BUFFER_LEN_CBC = 16765
FRAME_CBC = 1

VERSION_TLS1_2 = 0x0303
VERSION_TLS1_3 = 0x0304
CIPHER_AES_128_GCM = 1
CIPHER_AES_256_GCM = 2
CIPHER_CHACHA20_POLY1305 = 3
CIPHER_AES_192_GCM = 4
CIPHER_AES_128_CCM, CIPHER_AES_192_CCM, CIPHER_AES_256_CCM = 5, 6, 7
CIPHER_AES_128_CCM_8, CIPHER_AES_192_CCM_8, CIPHER_AES_256_CCM_8 = 8, 9, 10
CIPHER_ARIA_128_GCM, CIPHER_ARIA_192_GCM, CIPHER_ARIA_256_GCM = 11, 12, 13
CIPHER_ARIA_128_CCM, CIPHER_ARIA_192_CCM, CIPHER_ARIA_256_CCM = 14, 15, 16
CIPHER_CAMELLIA_128_GCM, CIPHER_CAMELLIA_192_GCM, CIPHER_CAMELLIA_256_GCM = 17, 18, 19
CIPHER_CAMELLIA_128_CCM, CIPHER_CAMELLIA_192_CCM, CIPHER_CAMELLIA_256_CCM = 20, 21, 22
KEYLEN = {1: 16, 2: 32, 3: 32, 4: 24, 5: 16, 6: 24, 7: 32, 8: 16, 9: 24, 10: 32, 11: 16, 12: 24, 13: 32,
          14: 16, 15: 24, 16: 32, 17: 16, 18: 24, 19: 32, 20: 16, 21: 24, 22: 32}
TAGLEN = {c: (8 if 8 <= c <= 10 else 16) for c in KEYLEN}
# AES-CBC + HMAC (key table, batch entry points and the _ex framing calls; mbedtls_amd/cbc.py).
# Not in KEYLEN / TAGLEN, which list the AEAD ids.
CIPHER_AES_128_CBC, CIPHER_AES_256_CBC = 23, 24
# each with one MAC: the 128-bit keys with MAC_SHA256, the 256-bit keys with MAC_SHA384 (25 is no cipher)
CIPHER_ARIA_128_CBC, CIPHER_ARIA_256_CBC, CIPHER_CAMELLIA_128_CBC, CIPHER_CAMELLIA_256_CBC = 26, 27, 28, 29
MAC_SHA1, MAC_SHA256, MAC_SHA384 = 1, 2, 3
MSG_APPLICATION_DATA = 23
MSG_CID = 25
CID_LEN_MAX = 32
ALG_SHA_256 = 0x02000009      # PSA_ALG_SHA_256
ALG_SHA_384 = 0x0200000a      # PSA_ALG_SHA_384
TLS13_CONTEXT_UNHASHED = 0
TLS13_CONTEXT_HASHED = 1
TLS13_PSK_EXTERNAL, TLS13_PSK_RESUMPTION = 0, 1             # ssl_tls13_keys.h:38-39
TLS_PRF_NONE, TLS_PRF_SHA384, TLS_PRF_SHA256 = 0, 1, 2      # mbedtls_tls_prf_types, ssl.h:1254-1256
IS_CLIENT, IS_SERVER = 0, 1                                 # MBEDTLS_SSL_IS_CLIENT / _SERVER

# ---- layouts -----------------------------------------------------------------
KEY_MATERIAL = np.dtype([("cipher", "u1"), ("tls_minor", "u1"), ("fixed_ivlen", "u1"),
                         ("taglen", "u1"), ("granularity", "u1"), ("reserved", "u1", 11),
                         ("iv", "u1", 16), ("key", "u1", 32)])
CBC_KEY_MATERIAL = np.dtype([("cipher", "u1"), ("tls_minor", "u1"), ("mac", "u1"), ("etm", "u1"),
                             ("reserved", "u1", 44), ("key", "u1", 32), ("mac_key", "u1", 48)])
assert CBC_KEY_MATERIAL.itemsize == 128
BATCH_REC = np.dtype([("buf_off", "<u8"), ("buf_len", "<u4"), ("data_offset", "<u4"),
                      ("data_len", "<u4"), ("slot", "<u4"), ("ctr", "u1", 8), ("type", "u1"),
                      ("ver", "u1", 2), ("cid_len", "u1"), ("cid_off", "<u4")], align=False)
BATCH_RES = np.dtype([("status", "<i4"), ("data_offset", "<u4"), ("data_len", "<u4"),
                      ("type", "u1"), ("cid_len", "u1"), ("reserved", "u1", 2)])
STREAM_IN = np.dtype([("off", "<u8"), ("len", "<u4"), ("slot", "<u4"), ("in_ctr", "u1", 8),
                      ("nb_zero", "u1"), ("reserved", "u1", 7)])
STREAM_IN_RES = np.dtype([("status", "<i4"), ("first", "<u4"), ("nrec", "<u4"), ("consumed", "<u4"),
                          ("in_ctr", "u1", 8), ("nb_zero", "u1"), ("reserved", "u1", 3), ("nparsed", "<u4")])
STREAM_OUT = np.dtype([("in_off", "<u8"), ("in_len", "<u4"), ("slot", "<u4"), ("out_off", "<u8"),
                       ("out_ctr", "u1", 8), ("max_frag", "<u4"), ("type", "u1"), ("reserved", "u1", 3)])
STREAM_OUT_RES = np.dtype([("status", "<i4"), ("first", "<u4"), ("nrec", "<u4"), ("out_len", "<u4"),
                           ("out_ctr", "u1", 8), ("nparsed", "<u4"), ("reserved", "u1", 4)])
TICKET = np.dtype([("off", "<u8"), ("len", "<u4"), ("clear_len", "<u4")])
TICKET_RES = np.dtype([("status", "<i4"), ("tlen", "<u4"), ("reserved", "<u4", 2)])
assert TICKET.itemsize == 16 and TICKET_RES.itemsize == 16
COOKIE_ITEM = np.dtype([("id_off", "<u8"), ("cookie_off", "<u8"), ("id_len", "<u4"), ("cookie_len", "<u4")])
CLIHLO = np.dtype([("off", "<u8"), ("id_off", "<u8"), ("out_off", "<u8"), ("len", "<u4"), ("id_len", "<u4"),
                   ("out_cap", "<u4"), ("reserved", "<u4")])
CLIHLO_RES = np.dtype([("status", "<i4"), ("olen", "<u4")])
assert COOKIE_ITEM.itemsize == 24 and CLIHLO.itemsize == 40 and CLIHLO_RES.itemsize == 8
# running handshake hashes (tlsrec_transcript_batch_update; mbedtls_amd/transcript.py)
TRANSCRIPT_RESET, TRANSCRIPT_SNAPSHOT, TRANSCRIPT_HRR = 1, 2, 4
TRANSCRIPT_STATE = np.dtype([("h", "<u8", 8), ("count", "<u8"), ("hash", "<u4"), ("reserved", "<u4"),
                             ("block", "u1", 128)])
TRANSCRIPT_SEG = np.dtype([("off", "<u8"), ("out_off", "<u8"), ("len", "<u4"), ("flags", "<u4")])
TRANSCRIPT_CONN = np.dtype([("state", "<u4"), ("first_seg", "<u4"), ("nseg", "<u4"), ("reserved", "<u4")])
assert TRANSCRIPT_STATE.itemsize == 208 and TRANSCRIPT_SEG.itemsize == 24 and TRANSCRIPT_CONN.itemsize == 16
STREAM_READ_REQ = np.dtype([("out_off", "<u8"), ("out_cap", "<u4"), ("reserved", "<u4")])
STREAM_READ_RES = np.dtype([("copied", "<u4"), ("records", "<u4"), ("left", "<u4"), ("reserved", "<u4")])
assert STREAM_READ_REQ.itemsize == 16 and STREAM_READ_RES.itemsize == 16
DGRAM = np.dtype([("off", "<u8"), ("len", "<u4"), ("reserved", "<u4")])
DTLS_IN = np.dtype([("window_top", "<u8"), ("window", "<u8"), ("first_dgram", "<u4"), ("ndgram", "<u4"),
                    ("slot", "<u4"), ("badmac_seen", "<u4"), ("badmac_limit", "<u4"), ("in_epoch", "<u2"),
                    ("cid_len", "u1"), ("flags", "u1"), ("nb_zero", "u1"), ("reserved", "u1", 7)])
DTLS_IN_RES = np.dtype([("window_top", "<u8"), ("window", "<u8"), ("status", "<i4"), ("first", "<u4"),
                        ("nrec", "<u4"), ("naccepted", "<u4"), ("dgrams_done", "<u4"), ("invalid_dgrams", "<u4"),
                        ("badmac_seen", "<u4"), ("nb_zero", "u1"), ("reserved", "u1", 3)])
assert DGRAM.itemsize == 16 and DTLS_IN.itemsize == 48 and DTLS_IN_RES.itemsize == 48
assert STREAM_IN.itemsize == 32 and STREAM_IN_RES.itemsize == 32
assert STREAM_OUT.itemsize == 40 and STREAM_OUT_RES.itemsize == 32
assert KEY_MATERIAL.itemsize == 64 and BATCH_REC.itemsize == 40 and BATCH_RES.itemsize == 16


class CTransform(ctypes.Structure):
    _fields_ = [("minlen", ctypes.c_size_t), ("ivlen", ctypes.c_size_t),
                ("fixed_ivlen", ctypes.c_size_t), ("maclen", ctypes.c_size_t),
                ("taglen", ctypes.c_size_t), ("iv_enc", ctypes.c_ubyte * 16),
                ("iv_dec", ctypes.c_ubyte * 16), ("tls_version", ctypes.c_int),
                ("cipher", ctypes.c_int), ("keylen", ctypes.c_size_t),
                ("key_enc", ctypes.c_ubyte * 32), ("key_dec", ctypes.c_ubyte * 32),
                ("slot_enc", ctypes.c_int32), ("slot_dec", ctypes.c_int32),
                ("granularity", ctypes.c_uint32), ("in_cid_len", ctypes.c_uint8),
                ("out_cid_len", ctypes.c_uint8), ("in_cid", ctypes.c_ubyte * 32),
                ("out_cid", ctypes.c_ubyte * 32)]


class CFrameOpts(ctypes.Structure):
    """tlsrec_frame_opts: the options of the tlsrec_stream_*_ex / tlsrec_dtls_*_ex calls"""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("cbc_ivs", ctypes.c_void_p)]


class CKeySet(ctypes.Structure):
    """struct mbedtls_ssl_key_set (library/ssl_misc.h:604-618)"""
    _fields_ = [("client_write_key", ctypes.c_ubyte * 32), ("server_write_key", ctypes.c_ubyte * 32),
                ("client_write_iv", ctypes.c_ubyte * 16), ("server_write_iv", ctypes.c_ubyte * 16),
                ("key_len", ctypes.c_size_t), ("iv_len", ctypes.c_size_t)]


class CTls12Conn(ctypes.Structure):
    """tlsrec_tls12_conn: one TLS 1.2 / DTLS 1.2 connection after its handshake (112 bytes)"""
    _fields_ = [("master", ctypes.c_ubyte * 48), ("randbytes", ctypes.c_ubyte * 64)]


class CTls12PmsConn(ctypes.Structure):
    """tlsrec_tls12_pms_conn: one TLS 1.2 / DTLS 1.2 connection at its key exchange (240 bytes)"""
    _fields_ = [("premaster", ctypes.c_ubyte * 128), ("randbytes", ctypes.c_ubyte * 64),
                ("session_hash", ctypes.c_ubyte * 48)]


class CTls13Secret(ctypes.Structure):
    """tlsrec_tls13_secret: one secret of the TLS 1.3 ladder (48 bytes, Hash.length used)"""
    _fields_ = [("secret", ctypes.c_ubyte * 48)]


class CTls13HsConn(ctypes.Structure):
    """tlsrec_tls13_hs_conn: one TLS 1.3 connection at its ServerHello (176 bytes)"""
    _fields_ = [("psk", ctypes.c_ubyte * 48), ("shared", ctypes.c_ubyte * 80), ("transcript", ctypes.c_ubyte * 48)]


class CTls13PskConn(ctypes.Structure):
    """tlsrec_tls13_psk_conn: one offered PSK at its ClientHello (144 bytes)"""
    _fields_ = [("psk", ctypes.c_ubyte * 48), ("binder_transcript", ctypes.c_ubyte * 48),
                ("hello_transcript", ctypes.c_ubyte * 48)]


_MD_MAX = ctypes.c_ubyte * 64      # MBEDTLS_TLS1_3_MD_MAX_SIZE


class CTls13EarlySecrets(ctypes.Structure):
    """mbedtls_ssl_tls13_early_secrets (library/ssl_misc.h:621-625)"""
    _fields_ = [("binder_key", _MD_MAX), ("client_early_traffic_secret", _MD_MAX),
                ("early_exporter_master_secret", _MD_MAX)]


class CTls13HandshakeSecrets(ctypes.Structure):
    """mbedtls_ssl_tls13_handshake_secrets (library/ssl_misc.h:627-630)"""
    _fields_ = [("client_handshake_traffic_secret", _MD_MAX), ("server_handshake_traffic_secret", _MD_MAX)]


class CTls13ApplicationSecrets(ctypes.Structure):
    """mbedtls_ssl_tls13_application_secrets (include/mbedtls/ssl.h:1085-1090)"""
    _fields_ = [("client_application_traffic_secret_N", _MD_MAX), ("server_application_traffic_secret_N", _MD_MAX),
                ("exporter_master_secret", _MD_MAX), ("resumption_master_secret", _MD_MAX)]


class CTicketKeys(ctypes.Structure):
    """the keys[2] / active fields of mbedtls_ssl_ticket_context"""
    _fields_ = [("slot", ctypes.c_uint32 * 2), ("name", (ctypes.c_uint8 * 4) * 2), ("active", ctypes.c_uint32)]


class CRecord(ctypes.Structure):
    _fields_ = [("ctr", ctypes.c_ubyte * 8), ("type", ctypes.c_ubyte), ("ver", ctypes.c_ubyte * 2),
                ("buf", ctypes.c_void_p), ("buf_len", ctypes.c_size_t),
                ("data_offset", ctypes.c_size_t), ("data_len", ctypes.c_size_t),
                ("cid_len", ctypes.c_ubyte), ("cid", ctypes.c_ubyte * 32)]


_I32, _U32 = ctypes.c_int32, ctypes.c_uint32


class GcmKnobs(ctypes.Structure):
    """tlsrec::GcmKnobs (csrc/tlsrec_plan.h): the TLSREC_GCM_* / TLSREC_GROUPED switches"""
    _fields_ = [("waves", _I32), ("wp", _I32), ("g5", _U32), ("treemul", _I32), ("hbuild", _U32), ("pair", _I32),
                ("grouped", _U32), ("srecs", _U32), ("pair_l", _I32), ("pair_small_min", _U32),
                ("pair_small_max", _U32), ("pair_big_max", _U32), ("lanes", _U32)]


class GcmPlanIn(ctypes.Structure):
    """tlsrec::GcmPlanIn: what the AES-GCM launch shape is decided from"""
    _fields_ = [(f, _U32) for f in ("n", "nloaded", "cu", "avg_bytes", "lanes", "nr", "has_cid", "coalesced",
                                    "keyrun")]


class GcmPlan(ctypes.Structure):
    """tlsrec::GcmPlan: lanes per record, waves, the launch log's waves code, GcmArgs rpw / tm / g5, grid"""
    _fields_ = [("L", _I32), ("waves", _I32), ("code", _I32), ("rpw", _U32), ("tm", _U32), ("g5", _U32),
                ("grid", _U32)]


class ChachaPlan(ctypes.Structure):
    _fields_ = [("L", _I32), ("rpw", _U32), ("grid", _U32)]


def gcm_plan(knobs=None, **inputs):
    """tlsrec__gcm_plan over GcmPlanIn(**inputs); knobs None = the process environment's switches"""
    f = load().tlsrec__gcm_plan
    f.restype, f.argtypes = None, [ctypes.c_void_p] * 3
    out = GcmPlan()
    f(ctypes.byref(GcmPlanIn(**inputs)), ctypes.byref(knobs) if knobs is not None else None, ctypes.byref(out))
    return out


def chacha_plan(n, cu, lanes_in, has_cid):
    f = load().tlsrec__chacha_plan
    f.restype, f.argtypes = None, [_U32, _U32, _U32, ctypes.c_int, ctypes.c_void_p]
    out = ChachaPlan()
    f(n, cu, lanes_in, has_cid, ctypes.byref(out))
    return out


class FrameKnobs(ctypes.Structure):
    """tlsrec::FrameKnobs: the TLSREC_RX_* / TLSREC_DTLS_STASH / TLSREC_STREAM_SRC switches"""
    _fields_ = [("groupwalk", _U32), ("fused_stream", _U32), ("rg", _I32), ("fused", _U32), ("stash", _U32),
                ("prefill", _U32), ("mailbox", _U32), ("stream_src", _U32)]


class StreamRxPlan(ctypes.Structure):
    _fields_ = [(f, _I32 if f == "G" else _U32) for f in ("fused", "G", "tile", "tiles", "count_grid", "emit_grid")]


class DtlsRxPlan(ctypes.Structure):
    _fields_ = [("fused", _U32), ("S", _I32), ("tiles", _U32)]


def _rx_plan(name, out):
    """tlsrec__stream_rx_plan / tlsrec__dtls_rx_plan; knobs None = the process environment's switches"""
    def plan(a, b, knobs=None):
        f, o = getattr(load(), name), out()
        f.restype, f.argtypes = None, [_U32, _U32, ctypes.c_void_p, ctypes.c_void_p]
        f(a, b, ctypes.byref(knobs) if knobs is not None else None, ctypes.byref(o))
        return o
    return plan


stream_rx_plan = _rx_plan("tlsrec__stream_rx_plan", StreamRxPlan)     # (nstreams, max_records, knobs=None)
dtls_rx_plan = _rx_plan("tlsrec__dtls_rx_plan", DtlsRxPlan)           # (nconns, ndgrams, knobs=None)


# every function include/tlsrec.h declares, with its signature
_VP, _U32, _INT, _SZ = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
SIGNATURES = {
    "tlsrec_transform_setup": (_INT, [_VP, _INT, _INT, _VP, _VP, _VP, _VP]),
    "tlsrec_transform_setup_ex": (_INT, [_VP, _INT, _INT, _VP, _VP, _VP, _VP, ctypes.c_uint]),
    "tlsrec_transform_setup_cbc": (_INT, [_VP, _INT, _INT, _INT, _INT, _VP, _VP, _VP, _VP]),
    "tlsrec_transform_free": (None, [_VP]),
    "tlsrec_transform_set_cid": (_INT, [_VP, _VP, _SZ, _VP, _SZ]),
    "tlsrec_keytab_set_cid": (_INT, [_VP, _U32, _VP, _SZ, _VP]),
    "tlsrec_encrypt_buf": (_INT, [_VP, _VP, _VP]),
    "tlsrec_decrypt_buf": (_INT, [_VP, _VP, _VP]),
    "tlsrec_keytab_create": (_INT, [ctypes.POINTER(_VP), _U32]),
    "tlsrec_keytab_load": (_INT, [_VP, _U32, _U32, _VP, _INT, _VP]),
    "tlsrec_keytab_capacity": (_U32, [_VP]),
    "tlsrec_keytab_free": (None, [_VP]),
    "tlsrec_batch_encrypt": (_INT, [_VP, _VP, _VP, _U32, _VP, _VP, _U32, _VP]),
    "tlsrec_batch_decrypt": (_INT, [_VP, _VP, _VP, _U32, _VP, _VP, _U32, _VP]),
    "tlsrec_batch_encrypt_sized": (_INT, [_VP, _VP, _VP, _U32, _VP, _VP, _U32, _VP]),
    "tlsrec_batch_decrypt_sized": (_INT, [_VP, _VP, _VP, _U32, _VP, _VP, _U32, _VP]),
    "tlsrec_host_batch_encrypt": (_INT, [_VP, _VP, _VP, _U32, _VP, _VP, _U32, ctypes.c_uint64]),
    "tlsrec_host_batch_decrypt": (_INT, [_VP, _VP, _VP, _U32, _VP, _VP, _U32, ctypes.c_uint64]),
    "tlsrec_frame_check": (_INT, [_INT, _VP, _VP, _VP, _VP, _VP]),
    "tlsrec_shard_bounds": (_INT, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _VP, _VP]),
    "tlsrec_device_check": (_INT, []),
    "tlsrec_tls13_hkdf_expand_label": (_INT, [_INT, _VP, _SZ, _VP, _SZ, _VP, _SZ, _VP, _SZ]),
    "tlsrec_tls13_derive_secret": (_INT, [_INT, _VP, _SZ, _VP, _SZ, _VP, _SZ, _INT, _VP, _SZ]),
    "tlsrec_tls13_evolve_secret": (_INT, [_INT, _VP, _VP, _SZ, _VP]),
    "tlsrec_tls13_make_traffic_keys": (_INT, [_INT, _VP, _VP, _SZ, _SZ, _SZ, _VP]),
    "tlsrec_tls13_exporter": (_INT, [_INT, _VP, _SZ, _VP, _SZ, _VP, _SZ, _VP, _SZ]),
    "tlsrec_tls13_update_traffic_secret": (_INT, [_INT, _VP, _VP]),
    "tlsrec_tls13_keytab_derive": (_INT, [_VP, _U32, _U32, _INT, _VP, _INT, _VP]),
    "tlsrec_tls13_derive_early_secrets": (_INT, [_INT, _VP, _VP, _SZ, _VP]),
    "tlsrec_tls13_derive_handshake_secrets": (_INT, [_INT, _VP, _VP, _SZ, _VP]),
    "tlsrec_tls13_derive_application_secrets": (_INT, [_INT, _VP, _VP, _SZ, _VP]),
    "tlsrec_tls13_derive_resumption_master_secret": (_INT, [_INT, _VP, _VP, _SZ, _VP]),
    "tlsrec_tls13_calc_finished": (_INT, [_INT, _VP, _VP, _VP, _VP]),
    "tlsrec_tls13_create_psk_binder": (_INT, [_INT, _VP, _SZ, _INT, _VP, _VP]),
    "tlsrec_tls13_keytab_derive_handshake": (_INT, [_VP, _U32, _U32, _INT, _U32, _U32, _VP, _VP, _VP, _VP, _VP]),
    "tlsrec_tls13_keytab_derive_application": (_INT, [_VP, _U32, _U32, _INT, _VP, _VP, _VP, _VP, _VP]),
    "tlsrec_tls13_batch_verify_data": (_INT, [_INT, _VP, _VP, _VP, _U32, _VP]),
    "tlsrec_tls13_batch_derive_secret": (_INT, [_INT, _VP, _SZ, _VP, _VP, _VP, _U32, _VP]),
    "tlsrec_tls13_batch_psk_binder": (_INT, [_INT, _U32, _INT, _VP, _VP, _VP, _VP, _U32, _VP]),
    "tlsrec_tls13_keytab_derive_early": (_INT, [_VP, _U32, _U32, _INT, _U32, _INT, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "tlsrec_tls13_batch_ticket_psk": (_INT, [_INT, _U32, _VP, _VP, _VP, _U32, _VP]),
    "tlsrec_tls13_batch_exporter": (_INT, [_INT, _VP, _VP, _SZ, _VP, _U32, _U32, _VP, _U32, _U32, _U32, _VP]),
    "tlsrec_tls12_batch_export_keying_material": (_INT, [_INT, _VP, _VP, _SZ, _VP, _U32, _U32, _INT, _VP, _U32, _U32,
                                                         _U32, _VP]),
    "tlsrec_tls_prf": (_INT, [_INT, _VP, _SZ, ctypes.c_char_p, _VP, _SZ, _VP, _SZ]),
    "tlsrec_tls12_compute_master": (_INT, [_INT, _VP, _SZ, _VP, _SZ, _INT, _VP]),
    "tlsrec_tls12_split_key_block": (_INT, [_INT, _VP, _SZ, _VP]),
    "tlsrec_tls12_make_keys": (_INT, [_INT, _INT, _VP, _VP, _VP]),
    "tlsrec_tls12_export_keying_material": (_INT, [_INT, _VP, _VP, _VP, _SZ, _VP, _SZ, _INT, _VP, _SZ]),
    "tlsrec_tls12_keytab_derive": (_INT, [_VP, _U32, _U32, _INT, _INT, _VP, _VP]),
    "tlsrec_tls12_batch_compute_master": (_INT, [_INT, _U32, _INT, _VP, _VP, _U32, _VP]),
    "tlsrec_tls12_calc_finished": (_INT, [_INT, _VP, _VP, _INT, _VP]),
    "tlsrec_tls12_batch_verify_data": (_INT, [_INT, _INT, _VP, _VP, _VP, _VP, _VP, _U32, _VP]),
    "tlsrec_tls12_psk_premaster": (_INT, [_VP, _SZ, _VP, _SZ, _VP, _SZ, _VP]),
    "tlsrec_ticket_write": (_INT, [_VP, _VP, _VP, _U32, _VP, _VP, _VP]),
    "tlsrec_ticket_parse": (_INT, [_VP, _VP, _VP, _U32, _VP, _VP, _VP]),
    "tlsrec_cookie_setup": (_INT, [ctypes.POINTER(_VP), _VP, _U32]),
    "tlsrec_cookie_set_timeout": (None, [_VP, _U32]),
    "tlsrec_cookie_free": (None, [_VP]),
    "tlsrec_cookie_batch_write": (_INT, [_VP, ctypes.c_uint64, _VP, _U32, _VP, _VP, _VP, _VP]),
    "tlsrec_cookie_batch_check": (_INT, [_VP, ctypes.c_uint64, _VP, _U32, _VP, _VP, _VP, _VP]),
    "tlsrec_cookie_write": (_INT, [_VP, ctypes.POINTER(_VP), _VP, _VP, _SZ]),
    "tlsrec_cookie_check": (_INT, [_VP, _VP, _SZ, _VP, _SZ]),
    "tlsrec_dtls_check_clihlo_cookies": (_INT, [_VP, ctypes.c_uint64, _VP, _U32, _VP, _VP, _VP, _VP, _VP]),
    "tlsrec_transcript_batch_update": (_INT, [_INT, _VP, _U32, _VP, _U32, _VP, _U32, _VP, ctypes.c_uint64, _VP,
                                              ctypes.c_uint64, _VP, _VP]),
    "tlsrec_x25519_batch_public": (_INT, [_VP, _VP, _U32, _U32, _VP]),
    "tlsrec_x25519_batch_shared": (_INT, [_VP, _VP, _U32, _VP, _U32, _VP, _U32, _VP]),
    "tlsrec_stream_decrypt": (_INT, [_VP, _VP, _U32, _VP, _VP, _VP, _U32, _VP, _VP, _VP]),
    "tlsrec_stream_read": (_INT, [_VP, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "tlsrec_stream_out_size": (ctypes.c_uint64, [_INT, _INT, _U32, ctypes.c_uint64, _U32]),
    "tlsrec_stream_encrypt": (_INT, [_VP, _VP, _U32, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP]),
    "tlsrec_dtls_decrypt": (_INT, [_VP, _VP, _U32, _VP, _U32, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP]),
    "tlsrec_dtls_out_size": (ctypes.c_uint64, [_INT, _U32, _U32, ctypes.c_uint64, _U32]),
    "tlsrec_dtls_encrypt": (_INT, [_VP, _VP, _U32, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP]),
    "tlsrec_stream_decrypt_ex": (_INT, [_VP, _VP, _U32, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP]),
    "tlsrec_stream_encrypt_ex": (_INT, [_VP, _VP, _U32, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP]),
    "tlsrec_dtls_decrypt_ex": (_INT, [_VP, _VP, _U32, _VP, _U32, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP]),
    "tlsrec_dtls_encrypt_ex": (_INT, [_VP, _VP, _U32, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP]),
    "tlsrec_stream_out_size_cbc": (ctypes.c_uint64, [_INT, _INT, ctypes.c_uint64, _U32]),
    "tlsrec_dtls_out_size_cbc": (ctypes.c_uint64, [_INT, _INT, _U32, ctypes.c_uint64, _U32]),
    "tlsrec_keytab_load_cbc": (_INT, [_VP, _U32, _U32, _VP, _INT, _VP]),
    "tlsrec_cbc_record_len": (_U32, [_INT, _INT, _U32]),
    "tlsrec_cbc_minlen": (_U32, [_INT, _INT]),
    "tlsrec_tls12_split_key_block_cbc": (_INT, [_INT, _INT, _VP, _SZ, _VP]),
    "tlsrec_tls12_make_keys_cbc": (_INT, [_INT, _INT, _INT, _VP, _VP, _VP]),
    "tlsrec_tls12_keytab_derive_cbc": (_INT, [_VP, _U32, _U32, _INT, _INT, _INT, _INT, _VP, _VP]),
    "tlsrec_version_string": (ctypes.c_char_p, []),
}

_lib = None


def load():
    """Load libtlsrec.so (HIP runtime linked).  torch, when importable, is
    imported first so that the process uses a single libamdhip64."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (shares its HIP runtime with us)
    except Exception:
        pass
    # TLSREC_LIBRARY: an alternative in-tree build of the same ABI (A/B runs)
    path = os.environ.get("TLSREC_LIBRARY") or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -m mbedtls_amd.build` "
                          "(there is no CPU fallback)")
    L = ctypes.CDLL(path)
    alt = path != LIB_PATH
    for name, (res, args) in SIGNATURES.items():
        if alt and not hasattr(L, name):
            continue          # an older A/B build may predate an entry point
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def tls13_exporter_blocks(hash_alg: int, label: bytes):
    """tlsrec__tls13_exporter_blocks (host only, no GPU): the padded inner message of the
    exporter's first Expand-Label as the batch kernel receives it.  Returns (status, words,
    nblk): 16 * nblk big-endian words, 32-bit under SHA-256 and 64-bit under SHA-384."""
    f = load().tlsrec__tls13_exporter_blocks
    f.restype, f.argtypes = _INT, [_INT, _VP, _SZ, _VP, _VP]
    words, nblk = (ctypes.c_uint64 * 80)(), _U32(0)
    r = f(hash_alg, bytes(label) if label is not None else None, len(label or b""), words, ctypes.byref(nblk))
    return r, list(words[:16 * nblk.value]), nblk.value


def x25519_host(scalar: bytes, point: bytes):
    """tlsrec__x25519_host (host only, no GPU; for the CPU tests, not a fallback): the ladder of
    csrc/tlsrec_x25519.h on the CPU.  Returns (32 output bytes, ok)."""
    f = load().tlsrec__x25519_host
    f.restype, f.argtypes = _INT, [_VP, ctypes.c_char_p, ctypes.c_char_p]
    assert len(scalar) == 32 and len(point) == 32
    out = ctypes.create_string_buffer(32)
    ok = f(out, bytes(scalar), bytes(point))
    return out.raw, ok


TEST_LIB_PATH = os.path.join(PKG, "libtlsrec_test.so")
_test_lib = None


def test_library():
    """The test-hooks build (tests/ only), loaded once, with the ABI's
    signatures bound."""
    global _test_lib
    if _test_lib is None:
        if not os.path.exists(TEST_LIB_PATH):
            raise ImportError(f"{TEST_LIB_PATH} is missing: build it with `python -m mbedtls_amd.build`")
        load()                       # torch first, as load() does
        L = ctypes.CDLL(TEST_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        L.tlsrec__test_launch_log_reset.restype = None
        L.tlsrec__test_launch_log_reset.argtypes = []
        L.tlsrec__test_launch_log_read.restype = _U32
        L.tlsrec__test_launch_log_read.argtypes = [_VP, _U32]
        _test_lib = L
    return _test_lib


# the launch log of the test-hooks build (csrc/tlsrec_internal.h TLSREC_LAUNCH_LOG)
LOG_GCM, LOG_CHACHA, LOG_ALT_GCM, LOG_CCM, LOG_BUCKET, LOG_SEND_FRAME, LOG_DTLS_RX_FRAME, LOG_STREAM_RX_FRAME = \
    1, 2, 3, 4, 5, 6, 7, 8
LOG_CBC = 9
LOG_CBC_KERNEL = 10          # follows every LOG_CBC entry: p0 1 = the wave-per-record kernel, 0 = the lane kernel
LAUNCH_LOG_ENTRY = np.dtype([("kind", "<i4"), ("p0", "<i4"), ("p1", "<i4"), ("p2", "<i4"), ("p3", "<i4")])


def launch_log_reset():
    """Forget the test library's launch log."""
    test_library().tlsrec__test_launch_log_reset()


def launch_log_read(cap=256):
    """The test library's last (up to cap) dispatch decisions, oldest first,
    as (kind, p0, p1, p2, p3) tuples of ints."""
    buf = np.zeros(cap, dtype=LAUNCH_LOG_ENTRY)
    n = test_library().tlsrec__test_launch_log_read(buf.ctypes.data, cap)
    return [tuple(int(x) for x in buf[i]) for i in range(n)]


class use_library:
    """Context manager for tests/: route every binding to another in-tree
    build of the same ABI for the duration -- the test-hooks build
    libtlsrec_test.so (-DTLSREC_TEST_HOOKS, the only one exporting
    tlsrec__test_*).  Objects (KeyTable, Transform) keep the library they were
    created with, so create them inside the block."""

    def __init__(self):
        self.saved = None

    def __enter__(self):
        global _lib
        L = test_library()
        self.saved, _lib = _lib, L
        return L

    def __exit__(self, *exc):
        global _lib
        _lib = self.saved
        return False
