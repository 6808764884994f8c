/*
 * tlsrec.h -- C ABI of the MI355X TLS record-protection engine (libtlsrec.so).
 *
 * Drop-in boundary for the AEAD record path of Mbed TLS 4.1.0:
 *
 *   reference (internal, library/ssl_misc.h:1724-1732)     this library
 *   ---------------------------------------------------    ----------------------
 *   int mbedtls_ssl_encrypt_buf(ssl, transform, rec)       tlsrec_encrypt_buf
 *       library/ssl_msg.c:784-1268
 *   int mbedtls_ssl_decrypt_buf(ssl, transform, rec)       tlsrec_decrypt_buf
 *       library/ssl_msg.c:1270-1834
 *   struct mbedtls_ssl_transform (ssl_misc.h:1073-1120)    tlsrec_transform
 *   mbedtls_record               (ssl_misc.h:1163-1188)    tlsrec_record
 *   mbedtls_ssl_tls13_populate_transform                   tlsrec_transform_setup
 *       (library/ssl_tls13_keys.c:922-1042) and the AEAD
 *       branch of ssl_tls12_populate_transform
 *       (library/ssl_tls.c:7768-7797)
 *   mbedtls_ssl_transform_free (ssl_msg.c:6084-6099)       tlsrec_transform_free
 *   psa_aead_encrypt / psa_aead_decrypt (TF-PSA-Crypto,    the HIP kernels behind
 *       called at ssl_msg.c:1043 and :1412)                 every entry point
 *
 * plus a device-resident batch extension (tlsrec_batch_encrypt/decrypt) that
 * applies the same per-record semantics to many records already in HBM, and a
 * key table (tlsrec_keytab_*) that holds per-connection keys on the GPU.
 *
 * Semantics and error codes are those of the reference: 0 on success or a
 * negative MBEDTLS_ERR_SSL_* value (include/mbedtls/ssl.h:40-125); the record
 * is transformed in place and its data_offset / data_len / type are updated
 * exactly as the reference updates them.  Supported: the AEAD suites
 * (AES-128/192/256-GCM, AES-128/192/256-CCM and CCM_8, ChaCha20-Poly1305,
 * ARIA-128/192/256-GCM and -CCM, Camellia-128/192/256-GCM and -CCM;
 * TLS 1.2 and 1.3, and DTLS 1.2 records with an RFC 9146 connection ID) on
 * every entry point, and the TLS 1.2 / DTLS 1.2 AES-128/256-CBC suites with
 * HMAC-SHA1 / -SHA256 / -SHA384 and the ARIA- and Camellia-128/256-CBC suites
 * with HMAC-SHA256 / -SHA384, MAC-then-encrypt or encrypt-then-MAC, on the
 * key table, the batch entry points (tlsrec_keytab_load_cbc below) and the
 * _ex forms of the stream and DTLS calls (tlsrec_frame_opts below).
 *
 * Every entry point that touches record data runs on the GPU; there is no CPU
 * fallback.  Without a usable HIP device they return
 * TLSREC_ERR_SSL_HW_ACCEL_FAILED (MBEDTLS_ERR_SSL_HW_ACCEL_FAILED).
 */
#ifndef TLSREC_H
#define TLSREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants (values of include/mbedtls/ssl.h) ---------------------- */
#define TLSREC_ERR_SSL_BAD_INPUT_DATA        (-135)    /* PSA_ERROR_INVALID_ARGUMENT, ssl.h:40 */
#define TLSREC_ERR_SSL_BUFFER_TOO_SMALL      (-138)    /* PSA_ERROR_BUFFER_TOO_SMALL, ssl.h:125 */
#define TLSREC_ERR_SSL_ALLOC_FAILED          (-141)    /* PSA_ERROR_INSUFFICIENT_MEMORY, ssl.h:101 */
#define TLSREC_ERR_SSL_FEATURE_UNAVAILABLE   (-0x7080) /* ssl.h:38 */
#define TLSREC_ERR_SSL_INVALID_MAC           (-0x7180) /* ssl.h:42 */
#define TLSREC_ERR_SSL_INVALID_RECORD        (-0x7200) /* ssl.h:44 */
#define TLSREC_ERR_SSL_HW_ACCEL_FAILED       (-0x7F80) /* ssl.h:103 */
#define TLSREC_ERR_SSL_INTERNAL_ERROR        (-0x6C00) /* ssl.h:117 */
#define TLSREC_ERR_SSL_UNEXPECTED_CID        (-0x6000) /* ssl.h:156 */

#define TLSREC_VERSION_TLS1_2   0x0303   /* MBEDTLS_SSL_VERSION_TLS1_2 */
#define TLSREC_VERSION_TLS1_3   0x0304   /* MBEDTLS_SSL_VERSION_TLS1_3 */

#define TLSREC_CIPHER_AES_128_GCM        1
#define TLSREC_CIPHER_AES_256_GCM        2
#define TLSREC_CIPHER_CHACHA20_POLY1305  3
/* the other AES AEADs of mbedtls_ssl_cipher_to_psa
 * (ssl_tls.c:2168-2363).  The _CCM_8 ids are the MBEDTLS_CIPHERSUITE_SHORT_TAG
 * suites (taglen 8: ssl_tls.c:7707-7708, ssl_tls13_keys.c:981-985). */
#define TLSREC_CIPHER_AES_192_GCM        4
#define TLSREC_CIPHER_AES_128_CCM        5
#define TLSREC_CIPHER_AES_192_CCM        6
#define TLSREC_CIPHER_AES_256_CCM        7
#define TLSREC_CIPHER_AES_128_CCM_8      8
#define TLSREC_CIPHER_AES_192_CCM_8      9
#define TLSREC_CIPHER_AES_256_CCM_8      10
/* ARIA-GCM (RFC 5794 block cipher; PSA_KEY_TYPE_ARIA + PSA_ALG_GCM in
 * mbedtls_ssl_cipher_to_psa, ssl_tls.c:2248-2289; the RFC 6209 TLS 1.2 suites) */
#define TLSREC_CIPHER_ARIA_128_GCM       11
#define TLSREC_CIPHER_ARIA_192_GCM       12
#define TLSREC_CIPHER_ARIA_256_GCM       13
/* ARIA-CCM (PSA_KEY_TYPE_ARIA + PSA_ALG_CCM, ssl_tls.c:2241-2282), 16-byte tag */
#define TLSREC_CIPHER_ARIA_128_CCM       14
#define TLSREC_CIPHER_ARIA_192_CCM       15
#define TLSREC_CIPHER_ARIA_256_CCM       16
/* Camellia-GCM / -CCM (RFC 3713 block cipher; PSA_KEY_TYPE_CAMELLIA with
 * PSA_ALG_GCM / PSA_ALG_CCM, ssl_tls.c:2297-2345; the RFC 6367 suites), 16-byte tag */
#define TLSREC_CIPHER_CAMELLIA_128_GCM   17
#define TLSREC_CIPHER_CAMELLIA_192_GCM   18
#define TLSREC_CIPHER_CAMELLIA_256_GCM   19
#define TLSREC_CIPHER_CAMELLIA_128_CCM   20
#define TLSREC_CIPHER_CAMELLIA_192_CCM   21
#define TLSREC_CIPHER_CAMELLIA_256_CCM   22
#define TLSREC_CIPHER_MAX                22      /* the last AEAD id */
/* AES-CBC + HMAC (MBEDTLS_SSL_MODE_CBC / _CBC_ETM); key table, batch entry
 * points and the _ex framing calls, loaded with tlsrec_keytab_load_cbc.  No TLS suite uses
 * AES-192-CBC. */
#define TLSREC_CIPHER_AES_128_CBC        23
#define TLSREC_CIPHER_AES_256_CBC        24
/* ARIA-CBC and Camellia-CBC + HMAC (RFC 6209 / RFC 5932 / RFC 6367 TLS 1.2
 * suites), through the same entry points.  Each id goes with ONE MAC, as every
 * suite of the reference pairs them: the 128-bit keys with TLSREC_MAC_SHA256,
 * the 256-bit keys with TLSREC_MAC_SHA384.  No suite uses a 192-bit key here.
 * Id 25 is no cipher. */
#define TLSREC_CIPHER_ARIA_128_CBC       26
#define TLSREC_CIPHER_ARIA_256_CBC       27
#define TLSREC_CIPHER_CAMELLIA_128_CBC   28
#define TLSREC_CIPHER_CAMELLIA_256_CBC   29
#define TLSREC_CIPHER_CBC_FIRST          23
#define TLSREC_CIPHER_CBC_LAST           29
/* record MACs of the CBC suites (no truncated HMAC, no MD5: the reference has
 * neither in a suite); maclen 20 / 32 / 48 */
#define TLSREC_MAC_SHA1                  1
#define TLSREC_MAC_SHA256                2
#define TLSREC_MAC_SHA384                3

#define TLSREC_MSG_APPLICATION_DATA  23      /* ssl.h:527 */
#define TLSREC_MSG_CID               25      /* MBEDTLS_SSL_MSG_CID, ssl.h:528 */
#define TLSREC_CID_LEN_MAX           32      /* MBEDTLS_SSL_CID_{IN,OUT}_LEN_MAX, ssl.h:423-429 */
#define TLSREC_OUT_CONTENT_LEN       16384   /* MBEDTLS_SSL_OUT_CONTENT_LEN, ssl.h:409 */
#define TLSREC_PADDING_GRANULARITY   16      /* MBEDTLS_SSL_CID_TLS1_3_PADDING_GRANULARITY, ssl.h:432 */

/* ---- single-record API (host buffers) --------------------------------- */

/* AEAD fields of struct mbedtls_ssl_transform, with raw key bytes and
 * device key-table slots in place of the PSA key ids psa_key_enc/dec.  A CBC +
 * HMAC transform (tlsrec_transform_setup_cbc) uses the same fields. */
typedef struct tlsrec_transform {
    size_t minlen;           /* min. ciphertext length */
    size_t ivlen;            /* 12; CBC: 16 */
    size_t fixed_ivlen;      /* 12, or 4 for TLS 1.2 GCM; CBC: 0 */
    size_t maclen;           /* 0 for AEAD; CBC: 20 / 32 / 48 */
    size_t taglen;           /* 16; CBC: 0 */
    unsigned char iv_enc[16];
    unsigned char iv_dec[16];
    int tls_version;         /* TLSREC_VERSION_* */
    int cipher;              /* TLSREC_CIPHER_* */
    size_t keylen;           /* 16, 24 or 32 */
    unsigned char key_enc[32];
    unsigned char key_dec[32];
    int32_t slot_enc;        /* device key slots (engine key table), -1 = none */
    int32_t slot_dec;
    uint32_t granularity;    /* MBEDTLS_SSL_CID_TLS1_3_PADDING_GRANULARITY (16) */
    /* DTLS 1.2 connection IDs (ssl_misc.h transform in_cid / out_cid); set
     * with tlsrec_transform_set_cid, zero after tlsrec_transform_setup */
    uint8_t in_cid_len;
    uint8_t out_cid_len;
    unsigned char in_cid[TLSREC_CID_LEN_MAX];
    unsigned char out_cid[TLSREC_CID_LEN_MAX];
} tlsrec_transform;

/* mbedtls_record (ssl_misc.h:1163-1188). */
typedef struct tlsrec_record {
    uint8_t ctr[8];          /* implicit sequence number (DTLS: epoch + seq), big endian */
    uint8_t type;            /* record content type */
    uint8_t ver[2];          /* version as on the wire */
    unsigned char *buf;      /* host buffer enclosing the record content */
    size_t buf_len;
    size_t data_offset;
    size_t data_len;
    uint8_t cid_len;         /* connection ID of the record (0 = none) */
    unsigned char cid[TLSREC_CID_LEN_MAX];
} tlsrec_record;

/* Populate `t` like mbedtls_ssl_tls13_populate_transform (TLS 1.3) or the
 * AEAD branch of ssl_tls12_populate_transform (TLS 1.2) and import both keys
 * into the engine's device key table.  iv_* point at 12 bytes (TLS 1.3,
 * ChaChaPoly) or at least fixed_ivlen bytes (TLS 1.2 GCM: 4). */
int tlsrec_transform_setup(tlsrec_transform *t, int tls_version, int cipher,
                           const unsigned char *key_enc, const unsigned char *key_dec,
                           const unsigned char *iv_enc, const unsigned char *iv_dec);
/* As tlsrec_transform_setup with an explicit TLS 1.3 padding granularity
 * (the reference's compile-time MBEDTLS_SSL_CID_TLS1_3_PADDING_GRANULARITY;
 * its record KATs are generated with 1). */
int tlsrec_transform_setup_ex(tlsrec_transform *t, int tls_version, int cipher,
                              const unsigned char *key_enc, const unsigned char *key_dec,
                              const unsigned char *iv_enc, const unsigned char *iv_dec,
                              unsigned granularity);
/* The CBC + HMAC branch of ssl_tls12_populate_transform (ssl_tls.c:7798-7847,
 * keys :7858-7886): cipher a TLSREC_CIPHER_*_CBC id, mac a TLSREC_MAC_*, etm 0
 * (MAC-then-encrypt) or 1 (encrypt-then-MAC, RFC 7366); key_* point at keylen
 * bytes, mac_* at maclen (20 / 32 / 48) bytes.  `t` gets ivlen 16, fixed_ivlen
 * and taglen 0, maclen, minlen = tlsrec_cbc_minlen(mac, etm), the cipher keys;
 * the MAC keys go into the device key slots only and are kept nowhere on the
 * host.  tlsrec_transform_set_cid, tlsrec_transform_free, tlsrec_encrypt_buf
 * and tlsrec_decrypt_buf then work on `t` as on an AEAD transform.
 * Errors, in this order and before the device is touched:
 * TLSREC_ERR_SSL_BAD_INPUT_DATA for a NULL pointer, then for a tls_version
 * other than TLS 1.2; TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for a (cipher, mac)
 * pair tlsrec_keytab_load_cbc does not accept; TLSREC_ERR_SSL_BAD_INPUT_DATA
 * for another etm.  Without a device: TLSREC_ERR_SSL_HW_ACCEL_FAILED, `t`
 * zeroed with both slots -1.
 *
 * The explicit IV of an encrypted record: the reference draws it with
 * psa_generate_random (ssl_msg.c:1124), tlsrec_encrypt_buf draws 16 bytes with
 * getrandom(2) and writes them at buf + data_offset - 16 (data_offset < 16:
 * nothing is drawn, the record gets the reference's BUFFER_TOO_SMALL of :1116).
 * The one divergence: a failed draw returns TLSREC_ERR_SSL_INTERNAL_ERROR, with
 * the record untouched, where the reference returns the PSA status. */
int tlsrec_transform_setup_cbc(tlsrec_transform *t, int tls_version, int cipher, int mac, int etm,
                               const unsigned char *key_enc, const unsigned char *key_dec,
                               const unsigned char *mac_enc, const unsigned char *mac_dec);
/* DTLS 1.2 connection IDs of a transform: in_cid (records it decrypts must
 * carry it, else TLSREC_ERR_SSL_UNEXPECTED_CID) and out_cid (records it
 * encrypts get it and become DTLSInnerPlaintext of type TLSREC_MSG_CID) --
 * what ssl_tls12_populate_transform copies from ssl->own_cid and the peer's
 * CID (library/ssl_tls.c).  Lengths <= TLSREC_CID_LEN_MAX, 0 = none.  Also
 * sets the CID of the transform's device key slots. */
int tlsrec_transform_set_cid(tlsrec_transform *t, const unsigned char *in_cid, size_t in_len,
                             const unsigned char *out_cid, size_t out_len);
/* Release the key slots and zeroize the transform. */
void tlsrec_transform_free(tlsrec_transform *t);

/* Same contract as mbedtls_ssl_encrypt_buf / mbedtls_ssl_decrypt_buf;
 * `ssl` is accepted for signature parity and only used for debugging in the
 * reference, it may be NULL. */
int tlsrec_encrypt_buf(void *ssl, tlsrec_transform *t, tlsrec_record *rec);
int tlsrec_decrypt_buf(const void *ssl, tlsrec_transform *t, tlsrec_record *rec);

/* ---- device key table -------------------------------------------------- */

/* One direction of one connection: the raw material a handshake produces
 * (what the RCCL broadcast carries).  64 bytes. */
typedef struct tlsrec_key_material {
    uint8_t cipher;          /* TLSREC_CIPHER_* */
    uint8_t tls_minor;       /* 3 = TLS 1.2, 4 = TLS 1.3 */
    uint8_t fixed_ivlen;     /* 12, or 4 for TLS 1.2 GCM */
    uint8_t taglen;          /* 16, or 8 for TLSREC_CIPHER_AES_*_CCM_8 */
    uint8_t granularity;     /* TLS 1.3 padding granularity, 0 = 16 (ssl.h:432) */
    uint8_t reserved[11];    /* zero (the device copy keeps the slot's CID length in [0]) */
    uint8_t iv[16];          /* static IV, first fixed_ivlen bytes used */
    uint8_t key[32];         /* 16, 24 or 32 bytes used */
} tlsrec_key_material;

typedef struct tlsrec_keytab tlsrec_keytab;

/* Device table of `capacity` slots on the current HIP device. */
int tlsrec_keytab_create(tlsrec_keytab **kt, uint32_t capacity);
/* Load `count` slots starting at `first` from `keys` (host memory, or device
 * memory when keys_on_device != 0) and expand them on the GPU (AES key
 * schedule, H = E_K(0), GHASH tables).  Enqueued on `stream` (hipStream_t,
 * NULL = default stream). */
int tlsrec_keytab_load(tlsrec_keytab *kt, uint32_t first, uint32_t count,
                       const tlsrec_key_material *keys, int keys_on_device,
                       void *stream);
/* Connection ID of slot `slot` (a transform direction: out_cid for an
 * encrypting slot, in_cid for a decrypting one); a (re)load resets it to
 * none.  Enqueued on `stream` and waited for. */
int tlsrec_keytab_set_cid(tlsrec_keytab *kt, uint32_t slot, const unsigned char *cid, size_t cid_len,
                          void *stream);
uint32_t tlsrec_keytab_capacity(const tlsrec_keytab *kt);
void tlsrec_keytab_free(tlsrec_keytab *kt);

/* ---- device-resident batch API ----------------------------------------- */

/* mbedtls_record with offsets into a device arena (40 bytes). */
typedef struct tlsrec_batch_rec {
    uint64_t buf_off;        /* rec->buf = arena + buf_off */
    uint32_t buf_len;
    uint32_t data_offset;
    uint32_t data_len;
    uint32_t slot;           /* key-table slot = the transform direction */
    uint8_t  ctr[8];         /* sequence number, big endian */
    uint8_t  type;
    uint8_t  ver[2];
    uint8_t  cid_len;        /* decrypt: the record's connection ID length (0 = none) */
    uint8_t  cid_off[4];     /* decrypt: its bytes at in_arena + buf_off + cid_off
                                (little-endian u32; the DTLS header holds them) */
} tlsrec_batch_rec;

/* The fields of the record after the call, plus its status (16 bytes). */
typedef struct tlsrec_batch_res {
    int32_t  status;         /* 0 or MBEDTLS_ERR_SSL_* */
    uint32_t data_offset;
    uint32_t data_len;
    uint8_t  type;
    uint8_t  cid_len;        /* encrypt: rec->cid_len as the reference leaves it
                                (the slot's CID once ssl_msg.c:874 has run) */
    uint8_t  reserved[2];
} tlsrec_batch_res;

/* Protect / unprotect `n` records.  `recs` and `res` are device arrays; the
 * record buffers live in `in_arena`; results are written to the same offsets
 * of `out_arena` (== in_arena for the reference's in-place behaviour).
 * Per-record semantics are those of mbedtls_ssl_encrypt_buf / _decrypt_buf
 * under the slot's key; a record naming a slot past the table or never
 * loaded gets TLSREC_ERR_SSL_BAD_INPUT_DATA and is left untouched.
 * Records may reference any mix of slots and ciphers in any order (the
 * engine groups them by key on the device); 128-byte aligned record buffers
 * avoid partial-line HBM writes.
 * lanes_per_record: 0 = auto, else lanes of a wavefront sharing one record:
 * 4/8/16/64 for AES-GCM, 1/2/4/8 for ChaCha20-Poly1305 (other values: auto).
 * Asynchronous on `stream` (hipStream_t, NULL = default stream); per-record
 * status lands in `res`. */
int tlsrec_batch_encrypt(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs,
                         tlsrec_batch_res *res, uint32_t n, const uint8_t *in_arena,
                         uint8_t *out_arena, uint32_t lanes_per_record, void *stream);
int tlsrec_batch_decrypt(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs,
                         tlsrec_batch_res *res, uint32_t n, const uint8_t *in_arena,
                         uint8_t *out_arena, uint32_t lanes_per_record, void *stream);

/* The same with the caller's mean record size (buf_len bytes, 0 = unknown)
 * as a launch hint: the host cannot read device-resident descriptors without
 * a sync, and with many keys of small records (<= 4 KiB, 12..127 per key)
 * the GCM kernels then take per-wave key passes at 2 or 4 lanes per record (the
 * stream / DTLS layers and the host pipeline pass the size themselves).
 * Results are identical with any hint; lanes are chosen automatically. */
int tlsrec_batch_encrypt_sized(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs,
                               tlsrec_batch_res *res, uint32_t n, const uint8_t *in_arena,
                               uint8_t *out_arena, uint32_t mean_record_bytes, void *stream);
int tlsrec_batch_decrypt_sized(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs,
                               tlsrec_batch_res *res, uint32_t n, const uint8_t *in_arena,
                               uint8_t *out_arena, uint32_t mean_record_bytes, void *stream);

/* Records in HOST memory (the socket-buffer boundary of ssl_msg.c:2058 /
 * :1855): the same per-record semantics as tlsrec_batch_*, with `recs` /
 * `res` host arrays and buf_off offsets into the host arenas in_arena /
 * out_arena (pinned memory, e.g. hipHostMalloc, gives the full PCIe rate).
 * The batch is cut into chunks of consecutive records of at most
 * chunk_bytes (0 = 64 MiB) of arena; each chunk's byte range is copied to
 * the device and protected there, copies and kernels overlapped on separate
 * streams.  Output: if out_arena is pinned host memory the device can
 * address (hipHostMalloc, hipHostRegister), the kernels write straight into
 * it -- exactly the bytes tlsrec_batch_* writes to its out_arena, so with
 * out_arena != in_arena the other bytes of a record are left as they were;
 * otherwise each chunk is protected in place on the device and its whole byte
 * range copied back to the same offsets of out_arena (gaps between records
 * carry the input bytes).  Records must be in ascending buf_off order and must not
 * overlap (else TLSREC_ERR_SSL_BAD_INPUT_DATA).  Synchronous: returns when
 * every result is in `res`. */
int tlsrec_host_batch_encrypt(tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                              uint32_t n, const uint8_t *in_arena, uint8_t *out_arena,
                              uint32_t lanes_per_record, uint64_t chunk_bytes);
int tlsrec_host_batch_decrypt(tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                              uint32_t n, const uint8_t *in_arena, uint8_t *out_arena,
                              uint32_t lanes_per_record, uint64_t chunk_bytes);

/* Host-only: run the record-framing checks of encrypt_buf / decrypt_buf
 * (everything decided before the AEAD, tlsrec_frame.h) for one batch record
 * under `km`.  Returns 1 if the record proceeds to the AEAD (aead_pos /
 * aead_len filled), 0 if it stops early (`early` holds the status and the
 * record fields the reference would leave).  Needs no GPU. */
int tlsrec_frame_check(int decrypt, const tlsrec_key_material *km, const tlsrec_batch_rec *rec,
                       tlsrec_batch_res *early, uint32_t *aead_pos, uint32_t *aead_len);

/* Host-only: rank `rank`'s contiguous share of a batch of n_records split
 * over `world` GPUs (one process per GPU): ranks differ
 * by at most one record, every record has exactly one owner.  The key table
 * reaches the ranks by a broadcast of rank 0's tlsrec_key_material array
 * (ncclBroadcast over RCCL/xGMI) followed by tlsrec_keytab_load with
 * keys_on_device = 1 -- tests/c/mgpu_shard.c shows the sequence. */
int tlsrec_shard_bounds(uint64_t n_records, uint32_t rank, uint32_t world, uint64_t *start, uint64_t *count);

/* ---- TLS 1.3 key schedule (library/ssl_tls13_keys.c) --------------------
 * HKDF-SHA256/384 on the GPU: the reference's single-shot functions with the
 * same arguments and return codes, plus a batch that derives many
 * connections' record keys straight into a device key table.  Hash
 * identifiers are the psa_algorithm_t values the reference passes. */
#define TLSREC_ALG_SHA_256   0x02000009   /* PSA_ALG_SHA_256 */
#define TLSREC_ALG_SHA_384   0x0200000a   /* PSA_ALG_SHA_384 */
#define TLSREC_TLS13_CONTEXT_UNHASHED 0   /* MBEDTLS_SSL_TLS1_3_CONTEXT_UNHASHED, ssl_tls13_keys.h:35 */
#define TLSREC_TLS13_CONTEXT_HASHED   1   /* MBEDTLS_SSL_TLS1_3_CONTEXT_HASHED, ssl_tls13_keys.h:36 */

/* struct mbedtls_ssl_key_set, library/ssl_misc.h:604-618 */
typedef struct tlsrec_key_set {
    unsigned char client_write_key[32];
    unsigned char server_write_key[32];
    unsigned char client_write_iv[16];
    unsigned char server_write_iv[16];
    size_t key_len;
    size_t iv_len;
} tlsrec_key_set;

/* mbedtls_ssl_tls13_hkdf_expand_label, ssl_tls13_keys.c:138-217 (label
 * without the "tls13 " prefix, <= 249 B; ctx <= 64 B; buf_len <= 255*64) */
int tlsrec_tls13_hkdf_expand_label(int hash_alg, const unsigned char *secret, size_t secret_len,
                                   const unsigned char *label, size_t label_len,
                                   const unsigned char *ctx, size_t ctx_len,
                                   unsigned char *buf, size_t buf_len);
/* mbedtls_ssl_tls13_derive_secret, ssl_tls13_keys.c:293-330 */
int tlsrec_tls13_derive_secret(int hash_alg, const unsigned char *secret, size_t secret_len,
                               const unsigned char *label, size_t label_len,
                               const unsigned char *ctx, size_t ctx_len, int ctx_hashed,
                               unsigned char *dstbuf, size_t dstbuf_len);
/* mbedtls_ssl_tls13_evolve_secret, ssl_tls13_keys.c:332-419 (secret_old may
 * be NULL: initial stage; input NULL or empty: all-zero IKM) */
int tlsrec_tls13_evolve_secret(int hash_alg, const unsigned char *secret_old,
                               const unsigned char *input, size_t input_len,
                               unsigned char *secret_new);
/* mbedtls_ssl_tls13_make_traffic_keys, ssl_tls13_keys.c:262-291 */
int tlsrec_tls13_make_traffic_keys(int hash_alg, const unsigned char *client_secret,
                                   const unsigned char *server_secret, size_t secret_len,
                                   size_t key_len, size_t iv_len, tlsrec_key_set *keys);
/* mbedtls_ssl_tls13_exporter, ssl_tls13_keys.c:1828-1858 */
int tlsrec_tls13_exporter(int hash_alg, const unsigned char *secret, size_t secret_len,
                          const unsigned char *label, size_t label_len,
                          const unsigned char *context_value, size_t context_len,
                          unsigned char *out, size_t out_len);
/* KeyUpdate (RFC 8446 7.2; label "traffic upd", ssl_tls13_keys.h:16):
 * next = HKDF-Expand-Label(secret, "traffic upd", "", Hash.length) */
int tlsrec_tls13_update_traffic_secret(int hash_alg, const unsigned char *secret,
                                       unsigned char *next);

/* One direction's traffic secret (client_application_traffic_secret_N or
 * server_...), 48 bytes; SHA-256 suites use the first 32. */
typedef struct tlsrec_tls13_secret {
    uint8_t secret[48];
} tlsrec_tls13_secret;

/* Batch: for each of `count` device-resident secrets, optionally first apply
 * a KeyUpdate in place (key_update != 0), then derive write_key / write_iv as
 * ssl_tls13_make_traffic_key does (ssl_tls13_keys.c:219-246) and load them
 * into slots first..first+count-1 of `kt` as TLS 1.3 keys of `cipher` (the
 * suite fixes the hash: AES-256-GCM -> SHA-384, others -> SHA-256; key
 * expansion and GHASH tables as tlsrec_keytab_load).  Asynchronous on
 * `stream`; the secrets buffer must stay valid until the stream reaches it. */
int tlsrec_tls13_keytab_derive(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                               tlsrec_tls13_secret *secrets, int key_update, void *stream);

/* ---- the rest of the TLS 1.3 ladder (RFC 8446 7.1) -----------------------
 * Single-shot: the four helpers of ssl_tls13_keys.c:421-650, the Finished MAC
 * and the PSK binder, with the reference's arguments.  `transcript` is the
 * transcript hash (MBEDTLS_SSL_TLS1_3_CONTEXT_HASHED).  A hash_alg that is no
 * PSA hash identifier returns TLSREC_ERR_SSL_INTERNAL_ERROR as the reference's
 * assertion does; a hash other than SHA-256 / SHA-384, or a NULL pointer,
 * TLSREC_ERR_SSL_BAD_INPUT_DATA.  Fields are MBEDTLS_TLS1_3_MD_MAX_SIZE =
 * PSA_HASH_MAX_SIZE = 64 bytes (ssl.h:672), the first Hash.length written. */
#define TLSREC_TLS13_PSK_EXTERNAL   0     /* MBEDTLS_SSL_TLS1_3_PSK_EXTERNAL, ssl_tls13_keys.h:38 */
#define TLSREC_TLS13_PSK_RESUMPTION 1     /* MBEDTLS_SSL_TLS1_3_PSK_RESUMPTION, ssl_tls13_keys.h:39 */

/* mbedtls_ssl_tls13_early_secrets, library/ssl_misc.h:621-625 */
typedef struct tlsrec_tls13_early_secrets {
    unsigned char binder_key[64];
    unsigned char client_early_traffic_secret[64];
    unsigned char early_exporter_master_secret[64];
} tlsrec_tls13_early_secrets;
/* mbedtls_ssl_tls13_handshake_secrets, library/ssl_misc.h:627-630 */
typedef struct tlsrec_tls13_handshake_secrets {
    unsigned char client_handshake_traffic_secret[64];
    unsigned char server_handshake_traffic_secret[64];
} tlsrec_tls13_handshake_secrets;
/* mbedtls_ssl_tls13_application_secrets, include/mbedtls/ssl.h:1085-1090 */
typedef struct tlsrec_tls13_application_secrets {
    unsigned char client_application_traffic_secret_N[64];
    unsigned char server_application_traffic_secret_N[64];
    unsigned char exporter_master_secret[64];
    unsigned char resumption_master_secret[64];
} tlsrec_tls13_application_secrets;

/* mbedtls_ssl_tls13_derive_early_secrets, ssl_tls13_keys.c:421-477 ("c e traffic",
 * "e exp master"; binder_key is left alone, as there) */
int tlsrec_tls13_derive_early_secrets(int hash_alg, const unsigned char *early_secret,
                                      const unsigned char *transcript, size_t transcript_len,
                                      tlsrec_tls13_early_secrets *derived);
/* mbedtls_ssl_tls13_derive_handshake_secrets, ssl_tls13_keys.c:479-543 */
int tlsrec_tls13_derive_handshake_secrets(int hash_alg, const unsigned char *handshake_secret,
                                          const unsigned char *transcript, size_t transcript_len,
                                          tlsrec_tls13_handshake_secrets *derived);
/* mbedtls_ssl_tls13_derive_application_secrets, ssl_tls13_keys.c:545-615
 * (resumption_master_secret is left alone) */
int tlsrec_tls13_derive_application_secrets(int hash_alg, const unsigned char *application_secret,
                                            const unsigned char *transcript, size_t transcript_len,
                                            tlsrec_tls13_application_secrets *derived);
/* mbedtls_ssl_tls13_derive_resumption_master_secret, ssl_tls13_keys.c:621-650
 * (writes resumption_master_secret only) */
int tlsrec_tls13_derive_resumption_master_secret(int hash_alg, const unsigned char *application_secret,
                                                 const unsigned char *transcript, size_t transcript_len,
                                                 tlsrec_tls13_application_secrets *derived);
/* ssl_tls13_calc_finished_core, ssl_tls13_keys.c:697-768: finished_key =
 * HKDF-Expand-Label(base_secret, "finished", "", Hash.length), out = HMAC(finished_key,
 * transcript); base_secret and transcript are Hash.length bytes, *out_len = Hash.length */
int tlsrec_tls13_calc_finished(int hash_alg, const unsigned char *base_secret,
                               const unsigned char *transcript, unsigned char *out, size_t *out_len);
/* mbedtls_ssl_tls13_create_psk_binder, ssl_tls13_keys.c:832-917 (without the ssl
 * context, which it uses for debug output only): Early Secret from the PSK, the
 * binder key under "res binder" (TLSREC_TLS13_PSK_RESUMPTION) or "ext binder" (any
 * other psk_type), then the Finished MAC over `transcript`; Hash.length bytes to result */
int tlsrec_tls13_create_psk_binder(int hash_alg, const unsigned char *psk, size_t psk_len, int psk_type,
                                   const unsigned char *transcript, unsigned char *result);

/* One TLS 1.3 connection at its ServerHello: 176 bytes, device-resident, only read */
typedef struct tlsrec_tls13_hs_conn {
    uint8_t psk[48];         /* psk_len bytes used */
    uint8_t shared[80];      /* (EC)DHE shared secret, shared_len bytes used */
    uint8_t transcript[48];  /* Hash(ClientHello..ServerHello), Hash.length bytes used */
} tlsrec_tls13_hs_conn;

/* Batch, handshake stage.  For each of `count` connections, in one kernel:
 *   Early Secret = Extract(0, PSK)            (psk_len == 0: Hash.length zero bytes, as
 *                                              tlsrec_tls13_evolve_secret takes a NULL input)
 *   Handshake Secret = Extract(Derive-Secret(., "derived", ""), shared)
 *                                             (shared_len == 0: zero bytes again, psk_ke)
 *   c hs traffic / s hs traffic over `transcript`     -> hs_traffic[2i], [2i + 1]
 *   their "finished" keys                             -> finished_keys[2i], [2i + 1] (may be NULL)
 *   their key / iv                                    -> slots first + 2i (client_write), first + 2i + 1
 *   Master Secret = Extract(Derive-Secret(., "derived", ""), 0)   -> master[i]
 * The slots are loaded as TLS 1.3 keys of `cipher` (tls_minor 4, fixed_ivlen 12); the
 * hash follows the cipher as in tlsrec_tls13_keytab_derive, which also names the
 * accepted cipher ids; slot numbering as tlsrec_tls12_keytab_derive.  psk_len (0..48)
 * and shared_len hold for the whole call.  The one divergence: shared_len is one of
 * 0, 32 (x25519, secp256r1), 48 (secp384r1), 56 (x448), 66 (secp521r1); the FFDH
 * groups' lengths are TLSREC_ERR_SSL_FEATURE_UNAVAILABLE here and stay with the
 * single-shot calls.  Every output is a device array; the first Hash.length bytes of
 * a 48-byte element are the value, the rest is written as zero.  Asynchronous on
 * `stream`, no host round trip; conns must stay valid until the stream reaches it.
 * Errors, in this order: TLSREC_ERR_SSL_BAD_INPUT_DATA for kt NULL, for conns,
 * hs_traffic or master NULL with count != 0, for psk_len > 48, for [first, first +
 * 2*count) overflowing or running past the table; TLSREC_ERR_SSL_FEATURE_UNAVAILABLE
 * for an unknown cipher, then for another shared_len.  count == 0 then returns 0. */
int tlsrec_tls13_keytab_derive_handshake(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                         uint32_t psk_len, uint32_t shared_len, const tlsrec_tls13_hs_conn *conns,
                                         tlsrec_tls13_secret *hs_traffic, tlsrec_tls13_secret *finished_keys,
                                         tlsrec_tls13_secret *master, void *stream);

/* Batch, application stage: from master[i] and transcripts[i] = Hash(ClientHello..server
 * Finished), c ap traffic -> app_traffic[2i], s ap traffic -> app_traffic[2i + 1], exp
 * master -> exporter[i] (may be NULL), and the two directions' key / iv into the slot
 * pair of the handshake stage.  app_traffic is in slot order, so a KeyUpdate of all of
 * them is tlsrec_tls13_keytab_derive(kt, first, 2*count, cipher, app_traffic, 1, stream).
 * Errors as above (master, transcripts or app_traffic NULL with count != 0). */
int tlsrec_tls13_keytab_derive_application(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                           const tlsrec_tls13_secret *master, const tlsrec_tls13_secret *transcripts,
                                           tlsrec_tls13_secret *app_traffic, tlsrec_tls13_secret *exporter,
                                           void *stream);
/* Batch: out[i] = HMAC(finished_keys[i], transcripts[i]), the verify_data of a Finished
 * message (RFC 8446 4.4.4).  TLSREC_ERR_SSL_BAD_INPUT_DATA for a hash other than
 * SHA-256 / SHA-384, then for a NULL array with count != 0; count == 0 returns 0. */
int tlsrec_tls13_batch_verify_data(int hash_alg, const tlsrec_tls13_secret *finished_keys,
                                   const tlsrec_tls13_secret *transcripts, tlsrec_tls13_secret *out,
                                   uint32_t count, void *stream);
/* Batch: out[i] = Derive-Secret(secrets[i], label, .) with the hashed context
 * transcripts[i] of Hash.length bytes, e.g. "res master" over Hash(ClientHello..client
 * Finished).  The batch takes a label of at most 12 bytes (every label of RFC 8446 7.1
 * fits); a longer one, or a NULL label with label_len != 0, is
 * TLSREC_ERR_SSL_BAD_INPUT_DATA, checked first; then as tlsrec_tls13_batch_verify_data. */
int tlsrec_tls13_batch_derive_secret(int hash_alg, const unsigned char *label, size_t label_len,
                                     const tlsrec_tls13_secret *secrets, const tlsrec_tls13_secret *transcripts,
                                     tlsrec_tls13_secret *out, uint32_t count, void *stream);

/* One offered PSK at its ClientHello: 144 bytes, device-resident, only read */
typedef struct tlsrec_tls13_psk_conn {
    uint8_t psk[48];                /* psk_len bytes used */
    uint8_t binder_transcript[48];  /* Hash(truncated ClientHello), Hash.length bytes used */
    uint8_t hello_transcript[48];   /* Hash(ClientHello); read only by tlsrec_tls13_keytab_derive_early */
} tlsrec_tls13_psk_conn;

/* Batch, PSK binder: what a server does once per resumed ClientHello,
 * ssl_tls13_offered_psks_check_binder_match (ssl_tls13_server.c:404-457) over
 * mbedtls_ssl_tls13_create_psk_binder (ssl_tls13_keys.c:832-917).  For each of `count`
 * connections, in one kernel:
 *   Early Secret = Extract(0, PSK)
 *   binder_key = Derive-Secret(., "res binder" | "ext binder", "")   (psk_type as in
 *                                             tlsrec_tls13_create_psk_binder: "res binder" for
 *                                             TLSREC_TLS13_PSK_RESUMPTION, "ext binder" otherwise)
 *   binder = the Finished MAC of binder_key over binder_transcript   -> binders[i] (may be NULL)
 *   match[i] = 1 if the first Hash.length bytes of offered[i] equal the binder, else 0
 * The compare ORs the XOR of every cell, with no early exit and no branch on the data, as
 * mbedtls_ct_memcmp does; bytes of offered[i] past Hash.length are not looked at.  offered
 * and match are both given or both NULL (a client computing its own binders passes NULL,
 * NULL); binders may be NULL only when match is given.  psk_len (1..48) and psk_type hold
 * for the whole call.  Every array is a device array; a 48-byte output element holds
 * Hash.length value bytes, the rest is written as zero; match is one uint32_t per
 * connection.  Asynchronous on `stream`, no host round trip; the inputs must stay valid
 * until the stream reaches the call.
 * Errors, in this order: TLSREC_ERR_SSL_BAD_INPUT_DATA for a hash other than SHA-256 /
 * SHA-384, for conns NULL with count != 0, for only one of offered and match given, for
 * binders and match both NULL with count != 0, for psk_len == 0 or psk_len > 48.
 * count == 0 then returns 0. */
int tlsrec_tls13_batch_psk_binder(int hash_alg, uint32_t psk_len, int psk_type,
                                  const tlsrec_tls13_psk_conn *conns, const tlsrec_tls13_secret *offered,
                                  tlsrec_tls13_secret *binders, uint32_t *match, uint32_t count, void *stream);

/* Batch, early stage: tlsrec_tls13_batch_psk_binder and, in the same kernel pass,
 * ssl_tls13_generate_early_key (ssl_tls13_keys.c:1086-1182) with
 * mbedtls_ssl_tls13_compute_early_transform (:1184-1225):
 *   c e traffic over hello_transcript                 -> early_traffic[i]
 *   e exp master over hello_transcript                -> early_exporter[i] (may be NULL: not computed)
 *   the key / iv of c e traffic                       -> slot first + i
 * One slot per connection, the client_write direction: a client writes 0-RTT records
 * with it, a server reads them.  The slots are loaded as TLS 1.3 keys of `cipher`
 * (tls_minor 4, fixed_ivlen 12); the hash follows the cipher as in
 * tlsrec_tls13_keytab_derive_handshake.  The slot is loaded whether or not the binder
 * matched: match[i] == 0 means the caller drops the connection and MUST NOT use slot
 * first + i, whose key then belongs to a PSK the peer has not proved it holds.
 * Errors, in this order: TLSREC_ERR_SSL_BAD_INPUT_DATA for kt NULL, for conns or
 * early_traffic NULL with count != 0, for the offered / match / binders rule and the
 * psk_len range of tlsrec_tls13_batch_psk_binder, for [first, first + count) overflowing
 * or running past the table; TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for an unknown cipher.
 * count == 0 then returns 0. */
int tlsrec_tls13_keytab_derive_early(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                     uint32_t psk_len, int psk_type, const tlsrec_tls13_psk_conn *conns,
                                     const tlsrec_tls13_secret *offered, tlsrec_tls13_secret *binders, uint32_t *match,
                                     tlsrec_tls13_secret *early_traffic, tlsrec_tls13_secret *early_exporter,
                                     void *stream);

/* Batch, ticket PSK (RFC 8446 4.6.1; ssl_tls13_server.c:3219-3230, ssl_tls13_client.c:2975-2990):
 *   psk[i] = HKDF-Expand-Label(res_master[i], "resumption", nonces[32 i .. 32 i + nonce_len), Hash.length)
 * between tlsrec_tls13_batch_derive_secret("res master") and tlsrec_ticket_write.  nonces
 * holds 32 bytes per ticket (MBEDTLS_SSL_TLS1_3_TICKET_NONCE_LENGTH), of which the first
 * nonce_len (0..32, the same for the whole call) are the nonce; the rest is not looked at.
 * The one divergence: a nonce longer than 32 bytes is TLSREC_ERR_SSL_FEATURE_UNAVAILABLE
 * here and stays with tlsrec_tls13_hkdf_expand_label.
 * Errors, in this order: TLSREC_ERR_SSL_BAD_INPUT_DATA for a hash other than SHA-256 /
 * SHA-384, for a NULL array with count != 0; TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for
 * nonce_len > 32.  count == 0 then returns 0. */
int tlsrec_tls13_batch_ticket_psk(int hash_alg, uint32_t nonce_len, const tlsrec_tls13_secret *res_master,
                                  const uint8_t *nonces /* count x 32 bytes */, tlsrec_tls13_secret *psk,
                                  uint32_t count, void *stream);

/* Batch, exporter (RFC 8446 7.5): mbedtls_ssl_tls13_exporter (ssl_tls13_keys.c:1828-1858),
 * what mbedtls_ssl_export_keying_material (ssl_tls.c:8969) runs for a TLS 1.3 session, for
 * each of `count` connections in one kernel:
 *   S1 = HKDF-Expand-Label(secrets[i], label, Hash(""), Hash.length)
 *   out[i * out_stride .. + out_len) = HKDF-Expand-Label(S1, "exporter", Hash(context i), out_len)
 * secrets is any array of tlsrec_tls13_secret: the `exporter` of
 * tlsrec_tls13_keytab_derive_application ("exp master"), or the `early_exporter` of
 * tlsrec_tls13_keytab_derive_early ("e exp master"), on the same stream with nothing in
 * between.  `label` is host memory, as in tlsrec_tls13_batch_derive_secret, and holds for the
 * whole call; secrets, contexts and out are device memory.  Connection i's context is
 * context_len bytes at contexts + i * context_stride; context_stride == 0 gives every
 * connection the one context at `contexts`; contexts == NULL with context_len == 0 is no
 * context (an empty context hashes to the same value).  Bytes [out_len, out_stride) of a row
 * are not touched; out may not overlap an input.  Asynchronous on `stream`, no host round
 * trip; the device inputs must stay valid until the stream reaches the call.
 * The one divergence: a context longer than 255 bytes is TLSREC_ERR_SSL_FEATURE_UNAVAILABLE
 * here and stays with tlsrec_tls13_exporter.
 * Errors, in this order: TLSREC_ERR_SSL_BAD_INPUT_DATA for a hash other than SHA-256 /
 * SHA-384; for secrets or out NULL, or contexts NULL with context_len != 0, when
 * count != 0; for label NULL with label_len != 0; for label_len > 249 (ssl_tls.c:8959); for
 * out_len > 8160 (MBEDTLS_SSL_EXPORT_MAX_KEY_LEN); for out_stride < out_len; for
 * context_stride != 0 && context_stride < context_len;
 * TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for context_len > 255.  count == 0 or out_len == 0 then
 * returns 0 and launches nothing; without a device TLSREC_ERR_SSL_HW_ACCEL_FAILED. */
int tlsrec_tls13_batch_exporter(int hash_alg, const tlsrec_tls13_secret *secrets,
                                const unsigned char *label, size_t label_len,
                                const uint8_t *contexts, uint32_t context_len, uint32_t context_stride,
                                uint8_t *out, uint32_t out_len, uint32_t out_stride,
                                uint32_t count, void *stream);

/* ---- TLS 1.2 / DTLS 1.2 key derivation (library/ssl_tls.c) ---------------
 * The TLS 1.2 PRF (RFC 5246 section 5, P_SHA256 / P_SHA384) on the GPU: the
 * reference's single-shot functions, and a batch that expands many
 * connections' master secrets straight into a device key table -- the first
 * half of ssl_tls12_populate_transform (ssl_tls.c:7750, :7858-7892), whose
 * second half is tlsrec_transform_setup.  TLS 1.2 fixes the hash per suite,
 * not per cipher (the *_SHA384 suites: AES-256-GCM, ARIA-256-GCM,
 * Camellia-256-GCM; AES-256-CCM and ChaCha20-Poly1305 use SHA-256), so `prf`
 * is explicit and every cipher works with either hash.
 * Return codes: a prf of TLSREC_TLS_PRF_NONE or any unknown value is
 * TLSREC_ERR_SSL_FEATURE_UNAVAILABLE (ssl_tls.c:465, decided before the GPU
 * is touched), a device failure TLSREC_ERR_SSL_HW_ACCEL_FAILED.  The one
 * divergence: the single-shot calls stage their inputs and output in a
 * 32 KiB device arena, and a call that does not fit returns
 * TLSREC_ERR_SSL_BAD_INPUT_DATA (PSA has no such limit). */
#define TLSREC_TLS_PRF_NONE    0   /* MBEDTLS_SSL_TLS_PRF_NONE,   ssl.h:1254 */
#define TLSREC_TLS_PRF_SHA384  1   /* MBEDTLS_SSL_TLS_PRF_SHA384, ssl.h:1255 */
#define TLSREC_TLS_PRF_SHA256  2   /* MBEDTLS_SSL_TLS_PRF_SHA256, ssl.h:1256 */
#define TLSREC_IS_CLIENT 0         /* MBEDTLS_SSL_IS_CLIENT */
#define TLSREC_IS_SERVER 1         /* MBEDTLS_SSL_IS_SERVER */

/* mbedtls_ssl_tls_prf, ssl_tls.c:465 (RFC 5246 section 5: P_hash over label ||
 * random; label is a C string).  slen == 0 is legal (ssl_tls.c:6117-6123);
 * dlen == 0 returns 0 and writes nothing. */
int tlsrec_tls_prf(int prf, const unsigned char *secret, size_t slen, const char *label,
                   const unsigned char *random, size_t rlen, unsigned char *dstbuf, size_t dlen);

/* ssl_compute_master, ssl_tls.c:6251 (non-PSK branch :6434): "master secret" over
 * client_random || server_random, or with extended_ms != 0 "extended master secret"
 * over the session hash (RFC 7627 section 4); master is 48 bytes */
int tlsrec_tls12_compute_master(int prf, const unsigned char *premaster, size_t pmslen,
                                const unsigned char *seed, size_t seed_len, int extended_ms,
                                unsigned char master[48]);

/* host-only, no GPU: the AEAD-branch split of the key block, ssl_tls.c:7858-7892
 * (mac_key_len = 0): client_write_key | server_write_key | client_write_iv | server_write_iv,
 * key_len = the cipher's, iv_len = fixed_ivlen (4 for GCM / CCM, 12 for ChaCha20-Poly1305).
 * A block shorter than 2 * key_len + 2 * iv_len is TLSREC_ERR_SSL_BAD_INPUT_DATA, an
 * unknown cipher TLSREC_ERR_SSL_FEATURE_UNAVAILABLE; unused bytes of `keys` are zero. */
int tlsrec_tls12_split_key_block(int cipher, const unsigned char *keyblk, size_t keyblk_len,
                                 tlsrec_key_set *keys);

/* PRF(master, "key expansion", randbytes) + the split; randbytes = server_random ||
 * client_random, i.e. handshake->randbytes after the swap at ssl_tls.c:6479-6488 */
int tlsrec_tls12_make_keys(int prf, int cipher, const unsigned char master[48],
                           const unsigned char randbytes[64], tlsrec_key_set *keys);

/* mbedtls_ssl_tls12_export_keying_material, ssl_tls.c:8886 (RFC 5705); randbytes as above
 * (the function un-swaps them, :8920-8925); context_len > 65535 -> BAD_INPUT_DATA */
int tlsrec_tls12_export_keying_material(int prf, const unsigned char master[48],
                                        const unsigned char randbytes[64],
                                        const char *label, size_t label_len,
                                        const unsigned char *context, size_t context_len,
                                        int use_context, unsigned char *out, size_t out_len);

/* One TLS 1.2 / DTLS 1.2 connection after its handshake, 112 bytes, device-resident */
typedef struct tlsrec_tls12_conn {
    uint8_t master[48];
    uint8_t randbytes[64];   /* server_random || client_random */
} tlsrec_tls12_conn;

/* Batch: for each of `count` connections run the key expansion and load
 * client_write into slot first + 2*i and server_write into slot first + 2*i + 1 of `kt`
 * as TLS 1.2 keys of `cipher` (tls_minor 3, fixed_ivlen 4 or 12, the cipher's taglen;
 * key expansion and GHASH tables as tlsrec_keytab_load).  A server endpoint
 * encrypts with the odd slot and decrypts with the even one; a client does
 * the reverse.  Asynchronous on `stream`; conns must stay valid until the
 * stream reaches it, and is only read.  No host round trip.
 * TLSREC_ERR_SSL_BAD_INPUT_DATA: kt NULL, conns NULL with count != 0, or
 * [first, first + 2*count) overflows or runs past the table;
 * TLSREC_ERR_SSL_FEATURE_UNAVAILABLE: unknown cipher (as
 * tlsrec_tls13_keytab_derive) or prf. */
int tlsrec_tls12_keytab_derive(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                               int prf, const tlsrec_tls12_conn *conns, void *stream);

/* One TLS 1.2 / DTLS 1.2 connection at its key exchange: 240 bytes, device-resident, only read */
typedef struct tlsrec_tls12_pms_conn {
    uint8_t premaster[128];    /* pms_len bytes used */
    uint8_t randbytes[64];     /* client_random || server_random (handshake->randbytes before the swap) */
    uint8_t session_hash[48];  /* extended_ms only: Hash(handshake messages), Hash.length bytes used */
} tlsrec_tls12_pms_conn;

/* Batch, master secret: ssl_compute_master (ssl_tls.c:6251-6452) for each of `count`
 * connections, in one kernel:
 *   master = PRF(premaster[0..pms_len), "master secret", randbytes)[0..48]
 * or with extended_ms != 0 (RFC 7627 section 4, ssl_tls.c:6284-6305)
 *   master = PRF(premaster[0..pms_len), "extended master secret", session_hash)[0..48]
 * where the session hash is Hash.length bytes, 32 under TLSREC_TLS_PRF_SHA256 and 48
 * under _SHA384.  out[i] is master || server_random || client_random: the swap of
 * ssl_tls.c:6479-6488 is done here, so `out` is the `conns` argument of
 * tlsrec_tls12_keytab_derive / _derive_cbc and of tlsrec_tls12_batch_verify_data on the
 * same stream, with nothing in between.  pms_len (1..128) and extended_ms hold for the
 * whole call; bytes of premaster past pms_len and of session_hash past Hash.length are
 * not looked at.  This covers the (EC)DHE and RSA premasters and the RFC 4279 forms
 * tlsrec_tls12_psk_premaster builds.
 * The one divergence: a premaster longer than 128 bytes (FFDH: the size of the group's
 * prime) is TLSREC_ERR_SSL_FEATURE_UNAVAILABLE here and stays with
 * tlsrec_tls12_compute_master.
 * The reference zeroizes handshake->premaster (:6447); conns is only read here, so the
 * caller wipes it once the stream has passed the call (a hipMemsetAsync on the same
 * stream does).  Both arrays are device arrays.  Asynchronous on `stream`, no host round
 * trip; conns must stay valid until the stream reaches the call.
 * Errors, in this order: TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for TLSREC_TLS_PRF_NONE or
 * an unknown prf (decided before the GPU is touched); TLSREC_ERR_SSL_BAD_INPUT_DATA for
 * conns or out NULL with count != 0, then for pms_len == 0;
 * TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for pms_len > 128.  count == 0 then returns 0 and
 * launches nothing. */
int tlsrec_tls12_batch_compute_master(int prf, uint32_t pms_len, int extended_ms,
                                      const tlsrec_tls12_pms_conn *conns,
                                      tlsrec_tls12_conn *out, uint32_t count, void *stream);

/* ssl_calc_finished_tls_generic, ssl_tls.c:7209-7261:
 *   out = PRF(master, "client finished" | "server finished", transcript_hash)[0..12]
 * `from` (TLSREC_IS_CLIENT / TLSREC_IS_SERVER) names the sender of the Finished message;
 * transcript_hash is Hash.length bytes.  Single-shot, like tlsrec_tls12_compute_master.
 * TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for the prf, then TLSREC_ERR_SSL_BAD_INPUT_DATA for
 * another `from` or a NULL pointer. */
int tlsrec_tls12_calc_finished(int prf, const unsigned char master[48], const unsigned char *transcript_hash,
                               int from, unsigned char out[12]);

/* Batch, Finished: tlsrec_tls12_calc_finished for each of `count` connections in one
 * kernel, and the check of mbedtls_ssl_parse_finished (ssl_tls.c:7488, mbedtls_ct_memcmp
 * at :7530):
 *   verify_data = PRF(conns[i].master, label of `from`, transcripts[i])[0..12]
 *                                                  -> verify[16 i .. 16 i + 12), then 4 zero bytes
 *   match[i] = 1 if offered[16 i .. 16 i + 12) equals it, else 0
 * Only `master` is read from a tlsrec_tls12_conn; a transcripts element holds Hash.length
 * bytes.  The compare ORs the XOR of the three words, with no early exit and no branch on
 * the data; bytes 12..15 of an offered element are not looked at.  offered and match are
 * both given or both NULL (an endpoint computing its own Finished passes NULL, NULL);
 * verify may be NULL only when match is given.  Every array is a device array; match is
 * one uint32_t per connection.  Asynchronous on `stream`, no host round trip.
 * Errors, in this order: TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for the prf;
 * TLSREC_ERR_SSL_BAD_INPUT_DATA for a `from` other than the two constants, for conns or
 * transcripts NULL with count != 0, for only one of offered and match given, for verify
 * and match both NULL with count != 0.  count == 0 then returns 0. */
int tlsrec_tls12_batch_verify_data(int prf, int from, const tlsrec_tls12_conn *conns,
                                   const tlsrec_tls13_secret *transcripts,
                                   const uint8_t *offered /* count x 16 bytes, 12 used */,
                                   uint8_t *verify /* count x 16 bytes */,
                                   uint32_t *match, uint32_t count, void *stream);

/* Batch, exporter (RFC 5705): mbedtls_ssl_tls12_export_keying_material (ssl_tls.c:8886-8936),
 * what mbedtls_ssl_export_keying_material (:8969) runs for a TLS 1.2 / DTLS 1.2 session, for
 * each of `count` connections in one kernel:
 *   out[i * out_stride .. + out_len) = PRF(conns[i].master, label,
 *       client_random || server_random [|| uint16(context_len) || context i])[0..out_len)
 * conns is the `out` of tlsrec_tls12_batch_compute_master on the same stream: randbytes is
 * server_random || client_random, and the kernel un-swaps it as :8920-8925 does.  `label` is
 * host memory and holds for the whole call (e.g. "EXTRACTOR-dtls_srtp", RFC 5764); conns,
 * contexts and out are device memory.  use_context == 0 is no context: the seed ends with the
 * randoms, and contexts, context_len and context_stride are not looked at.  With use_context
 * connection i's context is context_len bytes at contexts + i * context_stride
 * (context_stride == 0: the one context at `contexts` for all), and with context_len == 0 the
 * two bytes 00 00 are still appended (:8926-8929).  Bytes [out_len, out_stride) of a row are
 * not touched; out may not overlap an input.  Asynchronous on `stream`, no host round trip.
 * The one divergence: a context longer than 255 bytes is TLSREC_ERR_SSL_FEATURE_UNAVAILABLE
 * here and stays with tlsrec_tls12_export_keying_material.
 * Errors, in the order of tlsrec_tls13_batch_exporter, so that one label array serves a
 * terminator of both versions: TLSREC_ERR_SSL_BAD_INPUT_DATA for TLSREC_TLS_PRF_NONE or an
 * unknown prf; for conns or out NULL, or contexts NULL with use_context and
 * context_len != 0, when count != 0; for label NULL with label_len != 0; for
 * label_len > 249; for out_len > 8160; for out_stride < out_len; with use_context for
 * context_stride != 0 && context_stride < context_len;
 * TLSREC_ERR_SSL_FEATURE_UNAVAILABLE with use_context for context_len > 255.  count == 0 or
 * out_len == 0 then returns 0 and launches nothing; without a device
 * TLSREC_ERR_SSL_HW_ACCEL_FAILED. */
int tlsrec_tls12_batch_export_keying_material(int prf, const tlsrec_tls12_conn *conns,
                                              const char *label, size_t label_len,
                                              const uint8_t *contexts, uint32_t context_len, uint32_t context_stride,
                                              int use_context,
                                              uint8_t *out, uint32_t out_len, uint32_t out_stride,
                                              uint32_t count, void *stream);

/* Host-only, no GPU: the premaster of the PSK key exchanges (RFC 4279 section 2, what
 * PSA's PSK_TO_MS builds at ssl_tls.c:6307-6366),
 *   uint16(other_len) || other || uint16(psk_len) || psk
 * where `other` is the (EC)DHE shared secret, or for plain PSK (other NULL, other_len 0)
 * psk_len zero bytes.  *olen receives the length, the pms_len of
 * tlsrec_tls12_batch_compute_master.  TLSREC_ERR_SSL_BAD_INPUT_DATA for psk, out or olen
 * NULL, for psk_len == 0, for other NULL with other_len != 0 or a length past 65535;
 * TLSREC_ERR_SSL_BUFFER_TOO_SMALL when out_size is short (nothing written). */
int tlsrec_tls12_psk_premaster(const unsigned char *other, size_t other_len,
                               const unsigned char *psk, size_t psk_len,
                               unsigned char *out, size_t out_size, size_t *olen);

/* ---- CBC + HMAC slots: AES, ARIA, Camellia (TLS 1.2 / DTLS 1.2) ----------
 * (ARIA and Camellia: the ids 26..29 above, each with its one MAC; whatever
 * this section says of a CBC slot holds for them.  Sizes depend on the MAC and
 * the MAC order only: the block is 16 bytes for all three ciphers.)
 * The MBEDTLS_SSL_MODE_CBC and MBEDTLS_SSL_MODE_CBC_ETM branches of
 * mbedtls_ssl_encrypt_buf / _decrypt_buf (ssl_msg.c:906-968, :1080-1253,
 * :1435-1702, :1717-1801; transform setup ssl_tls.c:7799-7843) for records
 * of tlsrec_batch_encrypt / _decrypt, their _sized forms and
 * tlsrec_host_batch_*: a record naming a CBC slot gets the status,
 * data_offset, data_len, type and bytes the reference produces under that
 * transform.  A batch may mix CBC and AEAD slots freely.
 *
 * The one divergence -- the explicit IV on encrypt: the reference draws it
 * with psa_generate_random (ssl_msg.c:1124); the batch calls have no RNG
 * (tlsrec_encrypt_buf draws it on the host, above).  The
 * caller places the 16-byte IV at in_arena + buf_off + data_offset - 16 (as
 * the ticket API takes its IV); the engine encrypts under it and writes it to
 * the same offset of out_arena.  data_offset < 16 gives
 * TLSREC_ERR_SSL_BUFFER_TOO_SMALL where the reference checks it (:1116).
 *
 * Failures: status, data_offset and data_len are the reference's
 * (INVALID_MAC under encrypt-then-MAC: data_offset unchanged, data_len less
 * maclen; under MAC-then-encrypt: the values after :1572-1573, :1700 and
 * :1738).  The bytes of a record whose status is not 0 are unspecified;
 * nothing outside [buf_off, buf_off + buf_len) is ever written.
 *
 * The stream and DTLS framing layers take CBC slots through their _ex entry
 * points with TLSREC_FRAME_CBC set (tlsrec_frame_opts below); the plain
 * tlsrec_stream_* / tlsrec_dtls_* calls treat a CBC slot as a slot that was
 * never loaded.
 *
 * Batch key derivation for these suites is tlsrec_tls12_keytab_derive_cbc
 * (below).
 *
 * The single-record calls take CBC transforms made by
 * tlsrec_transform_setup_cbc (above); their records run through the coalescing
 * launch path, not the resident record server.
 *
 * Out of scope: session tickets treat a CBC slot as a slot that was never
 * loaded; the NULL cipher.
 * tlsrec_keytab_load, tlsrec_transform_setup, tlsrec_tls12_split_key_block,
 * tlsrec_tls12_make_keys, tlsrec_tls12_keytab_derive, tlsrec_tls13_keytab_derive, tlsrec_stream_out_size
 * and tlsrec_dtls_out_size answer ids 23, 24 and 26..29 as unknown ciphers. */

/* One direction of one connection, 128 bytes. */
typedef struct tlsrec_cbc_key_material {
    uint8_t cipher;          /* TLSREC_CIPHER_AES_128_CBC / _256_CBC, or _ARIA_ / _CAMELLIA_128_CBC / _256_CBC */
    uint8_t tls_minor;       /* 3 (TLS 1.2 / DTLS 1.2) */
    uint8_t mac;             /* TLSREC_MAC_*; ARIA / Camellia: _SHA256 with a 128-bit key, _SHA384 with a 256-bit key */
    uint8_t etm;             /* 0 = MAC-then-encrypt, 1 = encrypt-then-MAC (RFC 7366) */
    uint8_t reserved[44];    /* zero */
    uint8_t key[32];         /* 16 or 32 bytes used */
    uint8_t mac_key[48];     /* maclen bytes used */
} tlsrec_cbc_key_material;

/* tlsrec_keytab_load for CBC slots: the same contract (host or device
 * `keys`; host material is staged in a device buffer of the call's own and
 * the call waits for the key setup before it frees it, device material is
 * read once for the checks and the key setup enqueued on `stream`); the GPU expands the AES round keys of both
 * directions (ARIA, Camellia: the encryption and the decryption key array) and
 * the HMAC inner / outer midstates.  Unknown cipher or mac, or an ARIA /
 * Camellia id with another MAC than its suites': TLSREC_ERR_SSL_FEATURE_UNAVAILABLE; tls_minor != 3 or etm > 1:
 * TLSREC_ERR_SSL_BAD_INPUT_DATA.  A slot may be reloaded from AEAD to CBC and
 * back; tlsrec_keytab_set_cid works on a CBC slot (DTLS 1.2 connection IDs). */
int tlsrec_keytab_load_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count,
                           const tlsrec_cbc_key_material *keys, int keys_on_device, void *stream);

/* Host-only: bytes of explicit IV + ciphertext (+ MAC) a record of content_len
 * bytes becomes (without a connection ID); 0 for unknown ids. */
uint32_t tlsrec_cbc_record_len(int mac, int etm, uint32_t content_len);
/* Host-only: transform->minlen, ssl_tls.c:7822-7835; 0 for unknown ids. */
uint32_t tlsrec_cbc_minlen(int mac, int etm);

/* both directions' material of one connection */
typedef struct tlsrec_cbc_key_set {
    tlsrec_cbc_key_material client_write;
    tlsrec_cbc_key_material server_write;
} tlsrec_cbc_key_set;

/* Host-only: the mac_key_len != 0 layout of the key block, ssl_tls.c:7858-7886:
 * client_mac | server_mac | client_key | server_key.  Fills cipher, tls_minor 3,
 * mac, etm 0 (the caller sets it from the negotiated extension), key and
 * mac_key; the rest is zero.  A block shorter than 2 * maclen + 2 * key_len is
 * TLSREC_ERR_SSL_BAD_INPUT_DATA, an unknown cipher or mac
 * TLSREC_ERR_SSL_FEATURE_UNAVAILABLE. */
int tlsrec_tls12_split_key_block_cbc(int cipher, int mac, const unsigned char *keyblk, size_t keyblk_len,
                                     tlsrec_cbc_key_set *out);
/* PRF(master, "key expansion", randbytes) + the split above (arguments as
 * tlsrec_tls12_make_keys). */
int tlsrec_tls12_make_keys_cbc(int prf, int cipher, int mac, const unsigned char master[48],
                               const unsigned char randbytes[64], tlsrec_cbc_key_set *out);

/* tlsrec_tls12_keytab_derive for the CBC + HMAC suites: for each of `count`
 * connections run PRF(master, "key expansion", randbytes) for 2 * maclen +
 * 2 * key_len bytes on the GPU, split it as tlsrec_tls12_split_key_block_cbc
 * does and load client_write into slot first + 2*i and server_write into slot
 * first + 2*i + 1 as tlsrec_keytab_load_cbc loads them (tls_minor 3, `mac`,
 * `etm`).  `etm` (0 = MAC-then-encrypt, 1 = encrypt-then-MAC) holds for the
 * whole call: group connections by the negotiated extension.  `conns` is
 * device memory and only read.  Asynchronous on `stream`: no host
 * synchronisation, and no key material reaches the host; the derived records
 * pass through a device staging area of the table (capacity x 128 bytes,
 * allocated by the first call, freed with the table), which is zeroized on
 * `stream` right after the key setup.  A (re)loaded slot has no connection ID.
 * Every (cipher, mac, prf) combination tlsrec_tls12_make_keys_cbc accepts is
 * accepted (AES with every MAC, ARIA / Camellia with their suites' MAC).  Errors, in this order: TLSREC_ERR_SSL_BAD_INPUT_DATA for kt
 * NULL, conns NULL with count != 0, or [first, first + 2*count) overflowing or
 * running past the table; TLSREC_ERR_SSL_FEATURE_UNAVAILABLE for an unknown
 * cipher or mac or a pair no suite has, then for an unknown prf; TLSREC_ERR_SSL_BAD_INPUT_DATA for etm
 * other than 0 or 1.  count == 0 with valid arguments returns 0 and launches
 * nothing. */
int tlsrec_tls12_keytab_derive_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count,
                                   int cipher, int mac, int etm, int prf,
                                   const tlsrec_tls12_conn *conns, void *stream);

/* ---- TLS stream record layer --------------------------
 * Whole-connection framing on the device: received byte streams are split at
 * their 5-byte record headers, checked and decrypted in place; application
 * data is split into records, framed and encrypted into record streams.  Per
 * connection the result is what repeated ssl_get_next_record calls
 * (ssl_msg.c:4700-4900: ssl_parse_record_header :3561-3776,
 * ssl_prepare_record_content :3810-4017) or repeated mbedtls_ssl_write calls
 * (mbedtls_ssl_write_record :2648-2793) produce.  All arrays are device
 * memory; the calls synchronise `stream` once (to size the record batch). */
#define TLSREC_MAX_IN_RECORD  16421  /* header + body limit of mbedtls_ssl_fetch_input (AEAD-only build:
                                        MBEDTLS_SSL_IN_BUFFER_LEN 16429 minus the 8-byte in_hdr offset) */
#define TLSREC_OUT_BUF_SPACE  16416  /* out_buf_len - (out_iv - out_buf), ssl_msg.c:2688 (AEAD-only build) */
#define TLSREC_ERR_SSL_COUNTER_WRAPPING (-0x6B80)   /* ssl.h:119 */

/* One connection's received bytes, starting at a record header (ssl->in_hdr). */
typedef struct tlsrec_stream_in {
    uint64_t off;            /* first byte in the arena */
    uint32_t len;            /* bytes received (ssl->in_left) */
    uint32_t slot;           /* key slot of transform_in */
    uint8_t  in_ctr[8];      /* ssl->in_ctr */
    uint8_t  nb_zero;        /* ssl->nb_zero */
    uint8_t  reserved[7];
} tlsrec_stream_in;

typedef struct tlsrec_stream_in_res {
    int32_t  status;         /* 0: every complete record accepted (a trailing partial record waits);
                                else the error the reference returns for the first bad record */
    uint32_t first;          /* this connection's records are recs/res[first .. first+nparsed) */
    uint32_t nrec;           /* records accepted, in order; record k's plaintext is at
                                arena + recs[first+k].buf_off + res[first+k].data_offset */
    uint32_t consumed;       /* bytes of the accepted records (the next call starts there) */
    uint8_t  in_ctr[8];      /* ssl->in_ctr afterwards */
    uint8_t  nb_zero;
    uint8_t  reserved[3];
    uint32_t nparsed;        /* records framed (bytes of records after a failing one are unspecified) */
} tlsrec_stream_in_res;

/* `recs` / `res`: device arrays of max_records entries, filled by the call.
 * *nrecords (host, may be NULL) = records framed over all connections.
 * Returns TLSREC_ERR_SSL_BUFFER_TOO_SMALL (nothing decrypted) if the
 * connections hold more than max_records complete records. */
int tlsrec_stream_decrypt(const tlsrec_keytab *kt, const tlsrec_stream_in *streams, uint32_t nstreams,
                          uint8_t *arena, tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                          uint32_t max_records, tlsrec_stream_in_res *sres, uint32_t *nrecords,
                          void *stream);

/* Read side of mbedtls_ssl_read over the records tlsrec_stream_decrypt
 * accepted: per connection, ssl_read_application_data (ssl_msg.c:5627-5650)
 * in record order -- copy at most out_cap bytes of application data (type 23
 * records; other content types are the caller's) to out_arena + out_off and
 * zeroize the plaintext handed out; a record only partly consumed keeps its
 * tail (in_offt += n). */
typedef struct tlsrec_stream_read_req {
    uint64_t out_off;        /* the caller's buffer (buf of mbedtls_ssl_read) in out_arena */
    uint32_t out_cap;        /* len */
    uint32_t reserved;
} tlsrec_stream_read_req;

typedef struct tlsrec_stream_read_res {
    uint32_t copied;         /* bytes written to the caller's buffer */
    uint32_t records;        /* accepted records fully consumed (non-application ones included) */
    uint32_t left;           /* bytes still unread in the next record (in_msglen) */
    uint32_t reserved;
} tlsrec_stream_read_res;

int tlsrec_stream_read(const tlsrec_stream_in_res *sres, uint32_t nstreams, const tlsrec_batch_rec *recs,
                       const tlsrec_batch_res *res, uint8_t *arena, const tlsrec_stream_read_req *req,
                       uint8_t *out_arena, tlsrec_stream_read_res *rres, void *stream);

/* One connection's application data to send. */
typedef struct tlsrec_stream_out {
    uint64_t in_off;         /* plaintext in the input arena */
    uint32_t in_len;
    uint32_t slot;           /* key slot of transform_out */
    uint64_t out_off;        /* record stream destination in the output arena */
    uint8_t  out_ctr[8];     /* ssl->cur_out_ctr */
    uint32_t max_frag;       /* mbedtls_ssl_get_max_out_record_payload(); 0 = 16384 */
    uint8_t  type;           /* ssl->out_msgtype, normally 23 */
    uint8_t  reserved[3];
} tlsrec_stream_out;

typedef struct tlsrec_stream_out_res {
    int32_t  status;         /* 0 or the first record's error (COUNTER_WRAPPING after the record) */
    uint32_t first;          /* records recs/res[first .. first+nparsed) */
    uint32_t nrec;           /* records written */
    uint32_t out_len;        /* bytes of record stream written at out_off */
    uint8_t  out_ctr[8];     /* cur_out_ctr afterwards */
    uint32_t nparsed;
    uint8_t  reserved[4];
} tlsrec_stream_out_res;

/* Bytes of record stream `in_len` bytes of application data become (host
 * helper for sizing out_arena; 0 for an unsupported suite). */
uint64_t tlsrec_stream_out_size(int tls_version, int cipher, uint32_t granularity, uint64_t in_len,
                                uint32_t max_frag);
int tlsrec_stream_encrypt(const tlsrec_keytab *kt, const tlsrec_stream_out *streams, uint32_t nstreams,
                          const uint8_t *in_arena, uint8_t *out_arena, tlsrec_batch_rec *recs,
                          tlsrec_batch_res *res, uint32_t max_records, tlsrec_stream_out_res *sres,
                          uint32_t *nrecords, void *stream);

/* ---- DTLS 1.2 datagram record layer (DTLS branch) -------
 * The datagram-transport form of the same loops: received datagrams are
 * split at their 13-byte DTLS record headers (plus conf->cid_len CID bytes
 * for tls12_cid records) with the DTLS checks of ssl_parse_record_header
 * (ssl_msg.c:3561-3776: datagram holds the record, epoch, anti-replay window
 * :3248-3306), decrypted in place by the AEAD kernels, and ssl_get_next_record's
 * datagram rules applied per connection in arrival order (ssl_msg.c:4727-4873:
 * unexpected records skipped, a header error or a bad MAC drops the rest of
 * the datagram, badmac_limit, ignore_unexpected_cid) together with
 * ssl_prepare_record_content's DTLS post-rules (explicit sequence numbers, no
 * in_ctr step, mbedtls_ssl_dtls_replay_update).  Send writes one record per
 * mbedtls_ssl_write, each its own datagram (mbedtls_ssl_write_record,
 * :2648-2793: FE FD, epoch + 48-bit sequence, out_cid).  DTLS 1.2 only (the
 * reference has no DTLS 1.3): slots must hold TLS 1.2 keys. */
#define TLSREC_ERR_SSL_UNEXPECTED_RECORD (-0x6700)   /* ssl.h:136 */
#define TLSREC_ERR_SSL_EARLY_MESSAGE     (-0x6480)   /* ssl.h:146 */
#define TLSREC_ERR_SSL_CONN_EOF          (-0x7280)   /* ssl.h:46 */
/* MBEDTLS_SSL_IN_BUFFER_LEN / OUT_BUFFER_LEN of the AEAD-only build with DTLS
 * connection IDs (ssl_misc.h:300-392): 13 + 16 + 16 + 16 + 16384 + 32.  A
 * longer datagram is read truncated, as f_recv into that buffer would be. */
#define TLSREC_DTLS_MAX_DATAGRAM   16477
#define TLSREC_DTLS_OUT_BUFFER_LEN 16477
/* record dispositions (besides 0 = accepted and the MBEDTLS_ERR_SSL_* code
 * that skipped or dropped the record: UNEXPECTED_RECORD / EARLY_MESSAGE
 * (other epoch or replayed; skipped), INVALID_MAC (datagram dropped),
 * UNEXPECTED_CID (ignored), or the connection's fatal error) */
#define TLSREC_DTLS_DROPPED     1    /* discarded with the rest of its datagram */
#define TLSREC_DTLS_NOT_REACHED 2    /* after the connection's fatal error */
#define TLSREC_DTLS_ANTI_REPLAY            1   /* conf->anti_replay */
#define TLSREC_DTLS_IGNORE_UNEXPECTED_CID  2   /* conf->ignore_unexpected_cid */

/* One received datagram (one f_recv result) in the arena. */
typedef struct tlsrec_dgram {
    uint64_t off;
    uint32_t len;
    uint32_t reserved;
} tlsrec_dgram;

/* One connection's receive state (the mbedtls_ssl_context / config fields the
 * DTLS read loop uses) and its datagrams, in arrival order.  Datagram ranges
 * of different connections must not overlap. */
typedef struct tlsrec_dtls_in {
    uint64_t window_top;     /* ssl->in_window_top */
    uint64_t window;         /* ssl->in_window */
    uint32_t first_dgram;    /* dgrams[first_dgram .. first_dgram + ndgram) */
    uint32_t ndgram;
    uint32_t slot;           /* key slot of transform_in (TLS 1.2 key) */
    uint32_t badmac_seen;    /* ssl->badmac_seen */
    uint32_t badmac_limit;   /* conf->badmac_limit, 0 = no limit */
    uint16_t in_epoch;       /* ssl->in_epoch */
    uint8_t  cid_len;        /* conf->cid_len: CID length of incoming tls12_cid records */
    uint8_t  flags;          /* TLSREC_DTLS_ANTI_REPLAY | TLSREC_DTLS_IGNORE_UNEXPECTED_CID */
    uint8_t  nb_zero;        /* ssl->nb_zero */
    uint8_t  reserved[7];
} tlsrec_dtls_in;

typedef struct tlsrec_dtls_in_res {
    uint64_t window_top;     /* state afterwards */
    uint64_t window;
    int32_t  status;         /* 0, or the fatal error mbedtls_ssl_read returns (processing stops) */
    uint32_t first;          /* this connection's records are recs/res/disp[first .. first+nrec) */
    uint32_t nrec;           /* records a header walk finds in its datagrams, in order */
    uint32_t naccepted;      /* records with disposition 0: plaintext at
                                arena + recs[k].buf_off + res[k].data_offset, res[k].data_len, res[k].type */
    uint32_t dgrams_done;    /* datagrams fully processed before a fatal error */
    uint32_t invalid_dgrams; /* datagrams cut short by a header error (INVALID_RECORD) */
    uint32_t badmac_seen;
    uint8_t  nb_zero;
    uint8_t  reserved[3];
} tlsrec_dtls_in_res;

/* recs / res / disp: device arrays of max_records entries.  *nrecords (host,
 * may be NULL) = records listed over all connections.  Records skipped or
 * dropped keep unspecified bytes (the reference discards them too). */
int tlsrec_dtls_decrypt(const tlsrec_keytab *kt, const tlsrec_dtls_in *conns, uint32_t nconns,
                        const tlsrec_dgram *dgrams, uint32_t ndgrams, uint8_t *arena, tlsrec_batch_rec *recs,
                        tlsrec_batch_res *res, int32_t *disp, uint32_t max_records, tlsrec_dtls_in_res *cres,
                        uint32_t *nrecords, void *stream);

/* Bytes of datagrams `in_len` bytes of application data become under a TLS
 * 1.2 key with an out_cid of cid_len bytes (0 for an unsupported suite). */
uint64_t tlsrec_dtls_out_size(int cipher, uint32_t granularity, uint32_t cid_len, uint64_t in_len,
                              uint32_t max_frag);
/* tlsrec_stream_out with out_ctr = epoch (2 bytes) + 48-bit sequence number;
 * record k of a connection is one datagram: its header starts at
 * out_arena + recs[first + k].buf_off - 13 - cid_len and it is
 * 13 + cid_len + res[first + k].data_len bytes long. */
int tlsrec_dtls_encrypt(const tlsrec_keytab *kt, const tlsrec_stream_out *streams, uint32_t nstreams,
                        const uint8_t *in_arena, uint8_t *out_arena, tlsrec_batch_rec *recs,
                        tlsrec_batch_res *res, uint32_t max_records, tlsrec_stream_out_res *sres,
                        uint32_t *nrecords, void *stream);

/* ---- AES-CBC + HMAC connections in the stream and DTLS layers -------------
 * The four framing calls above with one more argument.  opts == NULL is the
 * plain call, byte for byte.  With TLSREC_FRAME_CBC a connection whose slot
 * holds a CBC key (tlsrec_keytab_load_cbc) is framed, protected and finished
 * as the reference does under that transform; every AEAD connection of the
 * call gets the results and bytes the plain call gives it.
 *
 * Limits follow the slot's kind.  An AEAD slot keeps TLSREC_MAX_IN_RECORD,
 * TLSREC_OUT_BUF_SPACE, TLSREC_DTLS_MAX_DATAGRAM and
 * TLSREC_DTLS_OUT_BUFFER_LEN, the AEAD-only build's values.  A CBC slot takes
 * those of a build with CBC and SHA-384 HMAC suites on (ssl_misc.h:283-301:
 * MBEDTLS_SSL_MAC_ADD 48, MBEDTLS_SSL_PADDING_ADD 256; :309-319 payload
 * overhead 16 + 48 + 256 (+ 16 with connection IDs); :382-400 buffer lengths):
 *   TLS:  13 + 320 + 16384 = 16717; less the 8-byte in_hdr offset, less the
 *         13 bytes before out_iv;
 *   DTLS: 13 + 336 + 16384 + 32 = 16765, in and out.
 *
 * Send, the explicit IV: the engine has no RNG (see the CBC section above).
 * Record recs[j] of a CBC connection takes cbc_ivs[16 j .. 16 j + 16); the
 * frame kernel places it at out_arena + recs[j].buf_off, where it becomes the
 * first 16 body bytes on the wire.  AEAD records ignore the array.  An
 * encrypt call with TLSREC_FRAME_CBC and cbc_ivs == NULL, unknown flag bits
 * or reserved != 0 returns TLSREC_ERR_SSL_BAD_INPUT_DATA before anything is
 * launched.  The decrypt calls do not read cbc_ivs. */
#define TLSREC_FRAME_CBC 1u
#define TLSREC_MAX_IN_RECORD_CBC        16709
#define TLSREC_OUT_BUF_SPACE_CBC        16704
#define TLSREC_DTLS_MAX_DATAGRAM_CBC    16765
#define TLSREC_DTLS_OUT_BUFFER_LEN_CBC  16765

typedef struct tlsrec_frame_opts {
    uint32_t flags;           /* TLSREC_FRAME_CBC: CBC slots are usable */
    uint32_t reserved;        /* zero */
    const uint8_t *cbc_ivs;   /* send only: device, 16 * max_records bytes */
} tlsrec_frame_opts;

int tlsrec_stream_decrypt_ex(const tlsrec_keytab *kt, const tlsrec_stream_in *streams, uint32_t nstreams,
                             uint8_t *arena, tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                             uint32_t max_records, tlsrec_stream_in_res *sres, uint32_t *nrecords,
                             void *stream, const tlsrec_frame_opts *opts);
int tlsrec_stream_encrypt_ex(const tlsrec_keytab *kt, const tlsrec_stream_out *streams, uint32_t nstreams,
                             const uint8_t *in_arena, uint8_t *out_arena, tlsrec_batch_rec *recs,
                             tlsrec_batch_res *res, uint32_t max_records, tlsrec_stream_out_res *sres,
                             uint32_t *nrecords, void *stream, const tlsrec_frame_opts *opts);
int tlsrec_dtls_decrypt_ex(const tlsrec_keytab *kt, const tlsrec_dtls_in *conns, uint32_t nconns,
                           const tlsrec_dgram *dgrams, uint32_t ndgrams, uint8_t *arena, tlsrec_batch_rec *recs,
                           tlsrec_batch_res *res, int32_t *disp, uint32_t max_records, tlsrec_dtls_in_res *cres,
                           uint32_t *nrecords, void *stream, const tlsrec_frame_opts *opts);
int tlsrec_dtls_encrypt_ex(const tlsrec_keytab *kt, const tlsrec_stream_out *streams, uint32_t nstreams,
                           const uint8_t *in_arena, uint8_t *out_arena, tlsrec_batch_rec *recs,
                           tlsrec_batch_res *res, uint32_t max_records, tlsrec_stream_out_res *sres,
                           uint32_t *nrecords, void *stream, const tlsrec_frame_opts *opts);
/* tlsrec_stream_out_size / tlsrec_dtls_out_size for a CBC slot (mac:
 * TLSREC_MAC_*, etm: 0 / 1); 0 for unknown ids or cid_len > TLSREC_CID_LEN_MAX. */
uint64_t tlsrec_stream_out_size_cbc(int mac, int etm, uint64_t in_len, uint32_t max_frag);
uint64_t tlsrec_dtls_out_size_cbc(int mac, int etm, uint32_t cid_len, uint64_t in_len, uint32_t max_frag);

/* ---- session tickets (library/ssl_ticket.c) ------------
 * mbedtls_ssl_ticket_write / mbedtls_ssl_ticket_parse for a batch of tickets
 * in device memory.  Ticket = key_name[4] || iv[12] || len16 || state ||
 * tag[16] (ssl_ticket.c:44-55); AEAD nonce = iv, AAD = the 18 header bytes.
 * The ticket keys are key-table slots holding an AES-GCM, AES-CCM (16-byte
 * tag) or ChaCha20-Poly1305 key (the cipher of mbedtls_ssl_ticket_setup). */
#define TLSREC_ERR_SSL_SESSION_TICKET_EXPIRED (-0x6D80)   /* ssl.h:111 */
#define TLSREC_TICKET_MIN_LEN 34                          /* TICKET_MIN_LEN, ssl_ticket.c:49-52 */

/* the keys[2] / active fields of mbedtls_ssl_ticket_context */
typedef struct tlsrec_ticket_keys {
    uint32_t slot[2];        /* key-table slots of keys[0], keys[1] */
    uint8_t  name[2][4];     /* their key names */
    uint32_t active;         /* ctx->active: the key new tickets use */
} tlsrec_ticket_keys;

typedef struct tlsrec_ticket {
    uint64_t off;            /* ticket start in the arena */
    uint32_t len;            /* write: end - start (space); parse: ticket length */
    uint32_t clear_len;      /* write: serialized session length; the state is at off + 18 and the caller's
                                random IV at off + 4 (psa_generate_random, ssl_ticket.c:255) */
} tlsrec_ticket;

typedef struct tlsrec_ticket_res {
    int32_t  status;         /* 0 or MBEDTLS_ERR_SSL_* as the reference returns it */
    uint32_t tlen;           /* write: *tlen; parse: clear_len (state decrypted in place at off + 18) */
    uint32_t reserved[2];
} tlsrec_ticket_res;

int tlsrec_ticket_write(const tlsrec_keytab *kt, const tlsrec_ticket_keys *keys, const tlsrec_ticket *tickets,
                        uint32_t n, uint8_t *arena, tlsrec_ticket_res *res, void *stream);
int tlsrec_ticket_parse(const tlsrec_keytab *kt, const tlsrec_ticket_keys *keys, const tlsrec_ticket *tickets,
                        uint32_t n, uint8_t *arena, tlsrec_ticket_res *res, void *stream);

/* ---- DTLS cookies (library/ssl_cookie.c, RFC 6347 4.2.1) ------------------
 * The stateless cookie exchange of a DTLS server for a batch of first-flight
 * datagrams: mbedtls_ssl_cookie_write / mbedtls_ssl_cookie_check
 * (ssl_cookie.c:117-179, :184-250) and mbedtls_ssl_check_dtls_clihlo_cookie
 * (ssl_msg.c:3322-3454), one item per lane, all under one secret.
 *     cookie = BE32(time) || HMAC-SHA256(key, BE32(time) || cli_id)[0..28)
 * (ssl_cookie.c:140-169).  HMAC-SHA256 truncated to 28 bytes is the only MAC:
 * the reference picks SHA-256 whenever it is compiled in (COOKIE_MD,
 * ssl_cookie.c:40-48; SHA-384 only in a build without it). */
#define TLSREC_ERR_SSL_DECODE_ERROR           (-0x7300)  /* ssl.h:48 */
#define TLSREC_ERR_SSL_HELLO_VERIFY_REQUIRED  (-0x6A80)  /* ssl.h:123 */
#define TLSREC_COOKIE_TIMEOUT 60                         /* MBEDTLS_SSL_COOKIE_TIMEOUT, ssl_cookie.h:27 */
#define TLSREC_COOKIE_LEN 32                             /* COOKIE_LEN = 4 + COOKIE_HMAC_LEN, ssl_cookie.c:56 */
#define TLSREC_DTLS_HVR_LEN 60                           /* 28 + TLSREC_COOKIE_LEN */

/* mbedtls_ssl_cookie_ctx (ssl_cookie.h:39-48): the two HMAC midstates of the
 * key (device memory; the raw key is not kept) and the timeout. */
typedef struct tlsrec_cookie_ctx tlsrec_cookie_ctx;   /* opaque */

/* mbedtls_ssl_cookie_init + _setup (ssl_cookie.c:58-111).  key == NULL: 32
 * bytes of getrandom(2), as psa_generate_key there; a caller's key is for
 * tests and for servers that share one secret.  timeout: seconds a cookie
 * stays valid, 0 = never expires (ssl_cookie.c:239).  HW_ACCEL_FAILED without
 * a usable device. */
int  tlsrec_cookie_setup(tlsrec_cookie_ctx **ctx, const unsigned char key[32], uint32_t timeout);
/* mbedtls_ssl_cookie_set_timeout (ssl_cookie.c:68-71) */
void tlsrec_cookie_set_timeout(tlsrec_cookie_ctx *ctx, uint32_t delay);
/* mbedtls_ssl_cookie_free (ssl_cookie.c:73-82): zeroes the device and host copies, then releases them; NULL is fine */
void tlsrec_cookie_free(tlsrec_cookie_ctx *ctx);

typedef struct tlsrec_cookie_item {
    uint64_t id_off;      /* client transport id (ssl->cli_id) in id_arena */
    uint64_t cookie_off;  /* write: 32 bytes of space; check: the received cookie, in cookie_arena */
    uint32_t id_len;      /* <= 255 */
    uint32_t cookie_len;  /* write: space (>= 32); check: received length */
} tlsrec_cookie_item;

/* f_cookie_write / f_cookie_check for n clients; every pointer but ctx is a
 * device pointer, offsets may be unaligned, `now` is the caller's
 * mbedtls_time(NULL).  status[i]:
 *   write: 0; BAD_INPUT_DATA for id_len > 255; BUFFER_TOO_SMALL for a space
 *          under 32 bytes (MBEDTLS_SSL_CHK_BUF_PTR, ssl_cookie.c:132), nothing written;
 *   check, in the order of ssl_cookie.c:194-242: BAD_INPUT_DATA for
 *          id_len > 255; -1 for cookie_len != 32; INVALID_MAC for a MAC
 *          mismatch (PSA_ERROR_INVALID_SIGNATURE through psa_to_ssl_errors,
 *          ssl_tls.c:2157-2166; compared in constant time); -1 when
 *          timeout != 0 && now - cookie_time > timeout (64-bit unsigned, the
 *          unsigned long of LP64: a cookie from the future is rejected); else 0.
 * A status the kernel did not reach reads INTERNAL_ERROR.  n == 0: 0, no launch. */
int tlsrec_cookie_batch_write(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_cookie_item *items, uint32_t n,
                              const uint8_t *id_arena, uint8_t *cookie_arena, int32_t *status, void *stream);
int tlsrec_cookie_batch_check(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_cookie_item *items, uint32_t n,
                              const uint8_t *id_arena, const uint8_t *cookie_arena, int32_t *status, void *stream);

/* The same for one client in host buffers, with time(NULL): the callback
 * types of mbedtls_ssl_conf_dtls_cookies (ssl.h:2935), so
 *     mbedtls_ssl_conf_dtls_cookies(conf, tlsrec_cookie_write, tlsrec_cookie_check, ctx)
 * works.  NULL ctx or cli_id: BAD_INPUT_DATA.  write advances *p by 32 on success. */
int tlsrec_cookie_write(void *ctx, unsigned char **p, unsigned char *end, const unsigned char *cli_id,
                        size_t cli_id_len);
int tlsrec_cookie_check(void *ctx, const unsigned char *cookie, size_t cookie_len, const unsigned char *cli_id,
                        size_t cli_id_len);

typedef struct tlsrec_clihlo {
    uint64_t off;       /* the datagram (record + handshake headers included) in `arena` */
    uint64_t id_off;    /* cli_id in `id_arena` */
    uint64_t out_off;   /* obuf in `out_arena` */
    uint32_t len;       /* in_len */
    uint32_t id_len;    /* <= 255 */
    uint32_t out_cap;   /* buf_len */
    uint32_t reserved;
} tlsrec_clihlo;

typedef struct tlsrec_clihlo_res { int32_t status; uint32_t olen; } tlsrec_clihlo_res;

/* mbedtls_ssl_check_dtls_clihlo_cookie (ssl_msg.c:3322-3454) for n datagrams
 * in one launch: parse, check the embedded cookie, write the
 * HelloVerifyRequest where it fails.  res[i].status:
 *   DECODE_ERROR            len < 61, in[0] != 22, epoch != 0, fragment_offset != 0,
 *                           61 + sid_len > len or 61 + sid_len + cookie_len > len (:3360-3393);
 *   0                       the cookie passes tlsrec_cookie_batch_check; olen = 0, nothing written;
 *   BUFFER_TOO_SMALL        it fails and out_cap < 28 (:3424);
 *   INTERNAL_ERROR          it fails and 28 <= out_cap < 60: f_cookie_write fails its buffer check
 *                           (:3436-3440); this call writes nothing then;
 *   HELLO_VERIFY_REQUIRED   otherwise: olen = 60 and the datagram of :3429-3451 at out_off -- bytes
 *                           0-24 of the input, msg_type 3, lengths 47 / 35 / 35, FE FF, 32 and
 *                           a fresh cookie stamped `now`.
 * An id_len > 255 makes both callbacks fail: after the DECODE_ERROR checks,
 * BUFFER_TOO_SMALL or INTERNAL_ERROR by out_cap alone.  Nothing outside
 * [out_off, out_off + 60) is written, and that only with HELLO_VERIFY_REQUIRED.
 * A result the kernel did not reach reads INTERNAL_ERROR, olen 0. */
int tlsrec_dtls_check_clihlo_cookies(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_clihlo *hellos, uint32_t n,
                                     const uint8_t *arena, const uint8_t *id_arena, uint8_t *out_arena,
                                     tlsrec_clihlo_res *res, void *stream);

/* ---- handshake transcripts (library/ssl_tls.c, ssl_tls13_generic.c) -------
 * The running handshake hash of many connections, kept in device memory and
 * advanced in batches; its digests land in the fields the batch calls above
 * read, so no transcript byte goes through the host between two of them.
 *
 *   reference                                              here
 *   ssl->handshake->fin_sha256_psa / fin_sha384_psa        tlsrec_transcript_state
 *   mbedtls_ssl_reset_checksum        (ssl_tls.c:838)      TLSREC_TRANSCRIPT_RESET
 *   update_checksum                   (ssl_tls.c:896-915)  a segment's bytes
 *   mbedtls_ssl_get_handshake_transcript (:5877-5925)      TLSREC_TRANSCRIPT_SNAPSHOT
 *   mbedtls_ssl_reset_transcript_for_hrr
 *                        (ssl_tls13_generic.c:1399-1441)   TLSREC_TRANSCRIPT_HRR
 *
 * Divergence: the reference keeps a SHA-256 and a SHA-384 operation side by
 * side until the suite is known (ssl_update_checksum_start, ssl_tls.c:869).
 * Here a state holds one hash and a call serves one hash; a client that has
 * to keep both keeps two state arrays and calls twice over the same segments. */
#define TLSREC_TRANSCRIPT_RESET     1u  /* before absorbing: the hash's initial state */
#define TLSREC_TRANSCRIPT_SNAPSHOT  2u  /* after absorbing: digest of everything hashed so far -> out_arena + out_off;
                                           the running state goes on (clone + finish) */
#define TLSREC_TRANSCRIPT_HRR       4u  /* last: the state becomes that of a fresh hash over
                                           FE 00 00 Hash.length || digest-so-far (message_hash, RFC 8446 4.4.1) */

/* One connection's running hash, device-resident: plain data in a fixed layout
 * (208 bytes, 8-byte aligned), so a state is cloned, saved or wiped with a
 * device memcpy / memset.  All-zero is "never reset": hash is no valid id. */
typedef struct tlsrec_transcript_state {
    uint64_t h[8];        /* chaining words; SHA-256 uses the low halves, the high halves are zero */
    uint64_t count;       /* bytes hashed so far; count % block size (64 / 128) is the fill level of block[] */
    uint32_t hash;        /* TLSREC_ALG_SHA_256 or TLSREC_ALG_SHA_384; anything else: needs a RESET */
    uint32_t reserved;    /* written as zero */
    uint8_t  block[128];  /* the partial block as message bytes; bytes at and past the fill level are zero
                             (SHA-256: all of block[64..128) ) */
} tlsrec_transcript_state;

typedef struct tlsrec_transcript_seg {    /* 24 bytes */
    uint64_t off;        /* bytes to absorb: arena[off .. off + len), any alignment, len may be 0 */
    uint64_t out_off;    /* SNAPSHOT: 48-byte element at out_arena + out_off, any alignment */
    uint32_t len;
    uint32_t flags;      /* TLSREC_TRANSCRIPT_* */
} tlsrec_transcript_seg;

typedef struct tlsrec_transcript_conn {   /* 16 bytes; the idiom of tlsrec_dtls_in / tlsrec_dgram */
    uint32_t state;      /* index into states */
    uint32_t first_seg;  /* segs[first_seg .. first_seg + nseg), applied in order */
    uint32_t nseg;
    uint32_t reserved;   /* zero */
} tlsrec_transcript_conn;

/* Advance nconns running hashes, one connection per lane.  hash_alg is
 * TLSREC_ALG_SHA_256 or TLSREC_ALG_SHA_384 (the ids of the tlsrec_tls13_*
 * calls) and holds for the whole call.  Per segment, in this order: RESET,
 * absorb len bytes, SNAPSHOT, HRR.  The bytes are hashed as they lie: the
 * 4-byte handshake headers of the wire (12-byte for DTLS) are part of what the
 * caller points at, as in update_checksum(ssl->in_msg, ssl->in_hslen).
 *
 * A snapshot element is 48 bytes -- Hash.length digest bytes, then zeros -- the
 * convention of tlsrec_tls13_secret, so out_off may aim at the transcript field
 * of a tlsrec_tls13_hs_conn, at binder_transcript / hello_transcript of a
 * tlsrec_tls13_psk_conn (a truncated ClientHello is two segments), at an
 * element of a `transcripts` array or at tlsrec_tls12_pms_conn.session_hash.
 *
 * status[i] is 0 or TLSREC_ERR_SSL_BAD_INPUT_DATA: state >= nstates;
 * first_seg + nseg past nsegs; reserved != 0; unknown flag bits; off + len
 * past arena_len; a SNAPSHOT with out_off + 48 past out_len; a first segment
 * without RESET on a state whose `hash` is not hash_alg (a zeroed state is
 * one).  Every segment of a connection is validated before its first byte is
 * absorbed: on an error the connection's state and every byte of out_arena
 * stay as they were, and its neighbours are unaffected.  A status the kernel
 * did not reach reads TLSREC_ERR_SSL_INTERNAL_ERROR (a prefill runs first on
 * the same stream).  Two conns of one call that name the same state, or
 * snapshots that overlap, are a caller error with an unspecified winner.
 *
 * All arrays are device memory; arena is only read, and no byte outside
 * [arena, arena + arena_len) is read; nothing is written but the named
 * states, the 48-byte snapshot elements and status.  Asynchronous on
 * `stream`, no host round trip.  The lanes of a wave run as long as the
 * longest of their 64 connections: a caller with very uneven message sizes
 * groups connections by size.
 *
 * Call-level errors, in this order, before the device is touched:
 * BAD_INPUT_DATA for another hash; for states, conns or status NULL with
 * nconns != 0; for segs NULL with nsegs != 0; for arena NULL with
 * arena_len != 0; for out_arena NULL with out_len != 0.  Then nconns == 0
 * returns 0 without a launch, and HW_ACCEL_FAILED follows without a gfx950
 * device. */
int tlsrec_transcript_batch_update(int hash_alg, tlsrec_transcript_state *states, uint32_t nstates,
                                   const tlsrec_transcript_conn *conns, uint32_t nconns,
                                   const tlsrec_transcript_seg *segs, uint32_t nsegs,
                                   const uint8_t *arena, uint64_t arena_len, uint8_t *out_arena, uint64_t out_len,
                                   int32_t *status /* nconns */, void *stream);

/* ---- X25519 key exchange in batches (x25519.hip) ------------------------
 * The (EC)DHE step in front of the key schedule, for the group x25519 (RFC 7748): what the
 * reference does through psa_generate_key + psa_export_public_key (ssl_tls13_generic.c:
 * 1566-1582) and psa_raw_key_agreement (ssl_tls13_keys.c:1457; ssl_tls12_server.c:2603-2631,
 * :3028).  One connection per lane.  Every array is a device array; both calls are
 * asynchronous on `stream` with no host round trip, and the inputs must stay valid until the
 * stream reaches the call.
 *
 * priv is count x 32 bytes, packed: 32 random bytes per connection, which the kernel clamps
 * (decodeScalar25519, RFC 7748 section 5).  The reference destroys the private key after the
 * agreement (psa_destroy_key, ssl_tls13_keys.c:1467); priv is only read here, so the caller
 * wipes it once the stream has passed the call (a hipMemsetAsync on the same stream does).
 * Generating the 32 bytes is the caller's.
 *
 * Each stride is at least 32.  Exactly 32 bytes per element are written, as the canonical
 * little-endian encoding; bytes between the elements are not touched.  Loads and stores are
 * 16-byte ones where the pointer and the stride are 16-byte aligned, byte ones otherwise.
 *
 * Errors of both calls, in this order, before the GPU is touched:
 * TLSREC_ERR_SSL_BAD_INPUT_DATA for a NULL array with count != 0, then for a stride below
 * 32.  count == 0 then returns 0 and launches nothing; without a gfx950 device
 * TLSREC_ERR_SSL_HW_ACCEL_FAILED.  There is no single-shot host-pointer form. */

/* pub[pub_stride * i .. + 32) = X25519(priv[32 i ..], 9)   (RFC 7748 section 5, section 6.1) */
int tlsrec_x25519_batch_public(const uint8_t *priv, uint8_t *pub, uint32_t pub_stride,
                               uint32_t count, void *stream);

/* out[out_stride * i .. + 32) = X25519(priv[32 i ..], peer[peer_stride * i ..]);
 * ok[i] = 1 unless those 32 bytes are all zero, then 0 (RFC 8446 section 7.4.2, RFC 7748
 * section 6.1).  Bit 255 of the peer's u-coordinate is masked; the non-canonical values
 * 2^255 - 19 .. 2^255 - 1 are accepted and reduced, as the RFC requires.  out_stride lets
 * the call write where the next one reads:
 *   out = (uint8_t *) conns + offsetof(tlsrec_tls13_hs_conn, shared), stride 176, for
 *         tlsrec_tls13_keytab_derive_handshake with shared_len 32;
 *   out = (uint8_t *) pms_conns, stride 240, for tlsrec_tls12_batch_compute_master with
 *         pms_len 32 (the TLS 1.2 ECDHE premaster is the raw 32 bytes);
 *   packed, stride 32.
 * ok is one uint32_t per connection (the convention of `match` in
 * tlsrec_tls12_batch_verify_data), computed from the OR of the eight output words with no
 * branch on the data.  It must not be NULL when count != 0: the RFCs' check is a MUST, so
 * the call does not let the caller skip it.  A connection with ok[i] == 0 has an all-zero
 * output: the caller drops it, and whatever the later stages derive for that connection
 * must not be trusted. */
int tlsrec_x25519_batch_shared(const uint8_t *priv, const uint8_t *peer, uint32_t peer_stride,
                               uint8_t *out, uint32_t out_stride, uint32_t *ok,
                               uint32_t count, void *stream);

/* ---- engine ------------------------------------------------------------- */
/* 0 if a gfx950 device is usable, else TLSREC_ERR_SSL_HW_ACCEL_FAILED. */
int tlsrec_device_check(void);
/* Library build string (kernel variants, arch). */
const char *tlsrec_version_string(void);

#ifdef __cplusplus
}
#endif
#endif /* TLSREC_H */
