/*
 * keysched.hip -- TLS 1.3 key schedule on the GPU.
 *
 * HKDF-SHA256 / HKDF-SHA384 (RFC 5869 over FIPS 180-4, HMAC per RFC 2104)
 * with the TLS 1.3 label encoding of library/ssl_tls13_keys.c:
 *
 *   reference                                   here
 *   ssl_tls13_hkdf_encode_label      :98-136    encode_label()       (host: framing only)
 *   mbedtls_ssl_tls13_hkdf_expand_label :138    tlsrec_tls13_hkdf_expand_label
 *   mbedtls_ssl_tls13_make_traffic_keys :262    tlsrec_tls13_make_traffic_keys
 *   mbedtls_ssl_tls13_derive_secret     :293    tlsrec_tls13_derive_secret
 *   mbedtls_ssl_tls13_evolve_secret     :332    tlsrec_tls13_evolve_secret
 *   mbedtls_ssl_tls13_exporter          :1828   tlsrec_tls13_exporter
 *   "traffic upd" (ssl_tls13_keys.h:16)         tlsrec_tls13_update_traffic_secret (RFC 8446 7.2)
 *   (batch)                                     tlsrec_tls13_keytab_derive: secrets in HBM ->
 *                                               key material -> key-table slots, no host round trip
 *   ..._derive_early / _handshake / _application_secrets,
 *   ..._derive_resumption_master_secret :421-650 tlsrec_tls13_derive_*_secrets, ..._resumption_master_secret
 *   ssl_tls13_calc_finished_core        :697    tlsrec_tls13_calc_finished
 *   mbedtls_ssl_tls13_create_psk_binder :832    tlsrec_tls13_create_psk_binder
 *   (batch)                                     tlsrec_tls13_keytab_derive_handshake, _application,
 *                                               tlsrec_tls13_batch_verify_data, _batch_derive_secret:
 *                                               the ladder from PSK / (EC)DHE secret to the application
 *                                               keys, written for its fixed shapes like the TLS 1.2 batch
 *   ssl_tls13_offered_psks_check_binder_match
 *                  (ssl_tls13_server.c:404-457)  tlsrec_tls13_batch_psk_binder
 *   ssl_tls13_generate_early_key :1086-1182,
 *   ..._compute_early_transform  :1184-1225     tlsrec_tls13_keytab_derive_early
 *   the "resumption" Expand-Label
 *                (ssl_tls13_server.c:3219-3230)  tlsrec_tls13_batch_ticket_psk
 *
 * Every hash, HMAC and HKDF step runs in a kernel; the host only encodes the
 * HkdfLabel byte string (length, "tls13 " + label, context length), moves
 * bytes and checks arguments the way the reference does.  One thread per
 * derivation: this is per-connection control work (a few SHA compressions),
 * not the bulk path, so lanes are independent and the message buffers live
 * in per-lane scratch.
 *
 * Also the TLS 1.2 / DTLS 1.2 key derivation of library/ssl_tls.c (the PRF of
 * RFC 5246 section 5; table at the host section below): the single-shot calls
 * as one more job of the same kernel, and a batch, tlsrec_tls12_keytab_derive,
 * whose kernel is written for its fixed shapes (word-oriented SHA-2 in
 * registers, HMAC midstates reused) instead of the byte-wise path above.
 *
 * And the DTLS cookie exchange (library/ssl_cookie.c, and
 * mbedtls_ssl_check_dtls_clihlo_cookie of library/ssl_msg.c) on the same
 * word-wise HMAC-SHA256 blocks: tlsrec_cookie_*, tlsrec_dtls_check_clihlo_cookies.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>
#include <time.h>

#include "tlsrec.h"
#include "tlsrec_frame.h"
#include "tlsrec_internal.h"
#include "tlsrec_sha.h"      /* round constants, ror32 / ror64, S256 / S512, sha_round, sha_compress */

namespace tlsks {

enum { H_SHA256 = 0, H_SHA384 = 1 };

/* The message block is kept as big-endian words (16 x 32 bit for SHA-256,
 * 16 x 64 bit for SHA-384), filled a byte at a time. */
struct Hash {
    uint32_t alg;
    uint32_t fill;            /* bytes in the current block */
    uint64_t total;           /* message bytes absorbed */
    uint64_t st[8];           /* SHA-256 uses the low 32 bits */
    uint64_t w[16];           /* SHA-256 uses the low 32 bits of w[0..15] */
};

__device__ __forceinline__ uint32_t blk_bytes(uint32_t alg) { return alg == H_SHA384 ? 128u : 64u; }
__device__ __forceinline__ uint32_t out_bytes(uint32_t alg) { return alg == H_SHA384 ? 48u : 32u; }

__device__ void compress(Hash &h)
{
    if (h.alg == H_SHA384) {
        uint64_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = h.w[i];
        uint64_t a = h.st[0], b = h.st[1], c = h.st[2], d = h.st[3], e = h.st[4], f = h.st[5], g = h.st[6],
                 k = h.st[7];
        for (int i = 0; i < 80; i++) {
            uint64_t wi;
            if (i < 16) {
                wi = w[i & 15];
            } else {
                const uint64_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
                wi = w[i & 15] + (ror64(w15, 1) ^ ror64(w15, 8) ^ (w15 >> 7)) + w[(i - 7) & 15] +
                     (ror64(w2, 19) ^ ror64(w2, 61) ^ (w2 >> 6));
                w[i & 15] = wi;
            }
            const uint64_t t1 = k + (ror64(e, 14) ^ ror64(e, 18) ^ ror64(e, 41)) + ((e & f) ^ (~e & g)) + kK512[i] + wi;
            const uint64_t t2 = (ror64(a, 28) ^ ror64(a, 34) ^ ror64(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
            k = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h.st[0] += a; h.st[1] += b; h.st[2] += c; h.st[3] += d;
        h.st[4] += e; h.st[5] += f; h.st[6] += g; h.st[7] += k;
    } else {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = (uint32_t) h.w[i];
        uint32_t a = (uint32_t) h.st[0], b = (uint32_t) h.st[1], c = (uint32_t) h.st[2], d = (uint32_t) h.st[3];
        uint32_t e = (uint32_t) h.st[4], f = (uint32_t) h.st[5], g = (uint32_t) h.st[6], k = (uint32_t) h.st[7];
        for (int i = 0; i < 64; i++) {
            uint32_t wi;
            if (i < 16) {
                wi = w[i & 15];
            } else {
                const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
                wi = w[i & 15] + (ror32(w15, 7) ^ ror32(w15, 18) ^ (w15 >> 3)) + w[(i - 7) & 15] +
                     (ror32(w2, 17) ^ ror32(w2, 19) ^ (w2 >> 10));
                w[i & 15] = wi;
            }
            const uint32_t t1 = k + (ror32(e, 6) ^ ror32(e, 11) ^ ror32(e, 25)) + ((e & f) ^ (~e & g)) + kK256[i] + wi;
            const uint32_t t2 = (ror32(a, 2) ^ ror32(a, 13) ^ ror32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            k = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h.st[0] = (uint32_t) (h.st[0] + a); h.st[1] = (uint32_t) (h.st[1] + b);
        h.st[2] = (uint32_t) (h.st[2] + c); h.st[3] = (uint32_t) (h.st[3] + d);
        h.st[4] = (uint32_t) (h.st[4] + e); h.st[5] = (uint32_t) (h.st[5] + f);
        h.st[6] = (uint32_t) (h.st[6] + g); h.st[7] = (uint32_t) (h.st[7] + k);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) h.w[i] = 0;
    h.fill = 0;
}

__device__ void hinit(Hash &h, uint32_t alg)
{
    /* FIPS 180-4 5.3.3 (SHA-256) and 5.3.4 (SHA-384) */
    const uint64_t iv256[8] = { 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19 };
    const uint64_t iv384[8] = { 0xcbbb9d5dc1059ed8ULL, 0x629a292a367cd507ULL, 0x9159015a3070dd17ULL,
                                0x152fecd8f70e5939ULL, 0x67332667ffc00b31ULL, 0x8eb44a8768581511ULL,
                                0xdb0c2e0d64f98fa7ULL, 0x47b5481dbefa4fa4ULL };
    h.alg = alg;
    h.fill = 0;
    h.total = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) h.st[i] = alg == H_SHA384 ? iv384[i] : iv256[i];
#pragma unroll
    for (int i = 0; i < 16; i++) h.w[i] = 0;
}

/* absorb one byte (no length accounting) */
__device__ __forceinline__ void put(Hash &h, uint32_t byte)
{
    const uint32_t wb = h.alg == H_SHA384 ? 8u : 4u;
    const uint32_t idx = h.fill / wb, sh = 8 * (wb - 1 - h.fill % wb);
    h.w[idx] |= (uint64_t) (byte & 0xff) << sh;
    if (++h.fill == blk_bytes(h.alg)) compress(h);
}

__device__ void update(Hash &h, const uint8_t *p, uint32_t n, uint8_t x = 0)
{
    for (uint32_t i = 0; i < n; i++) put(h, p[i] ^ x);
    h.total += n;
}

/* n copies of byte b (key padding) */
__device__ void update_fill(Hash &h, uint8_t b, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) put(h, b);
    h.total += n;
}

__device__ void finish(Hash &h, uint8_t *out)
{
    const uint64_t bits = h.total * 8;
    const uint32_t B = blk_bytes(h.alg), L = h.alg == H_SHA384 ? 16u : 8u;
    put(h, 0x80);
    while (h.fill != B - L) put(h, 0);
    for (uint32_t i = 0; i < L; i++) put(h, i < L - 8 ? 0u : (uint32_t) (bits >> (8 * (L - 1 - i))));
    const uint32_t n = out_bytes(h.alg);
    for (uint32_t i = 0; i < n; i++) {
        if (h.alg == H_SHA384) out[i] = (uint8_t) (h.st[i / 8] >> (56 - 8 * (i % 8)));
        else out[i] = (uint8_t) (h.st[i / 4] >> (24 - 8 * (i % 4)));
    }
}

/* HMAC (RFC 2104) with a key already reduced to <= one block. */
struct Hmac {
    Hash in;
    uint8_t k0[128];
    uint32_t klen;
};

__device__ void hmac_start(Hmac &m, uint32_t alg, const uint8_t *key, uint32_t klen)
{
    const uint32_t B = blk_bytes(alg);
    if (klen > B) {                     /* RFC 2104 2: hash keys longer than the block */
        Hash t;
        hinit(t, alg);
        update(t, key, klen);
        finish(t, m.k0);
        klen = out_bytes(alg);
    } else {
        for (uint32_t i = 0; i < klen; i++) m.k0[i] = key[i];
    }
    m.klen = klen;
    hinit(m.in, alg);
    update(m.in, m.k0, klen, 0x36);
    update_fill(m.in, 0x36, B - klen);
}

__device__ void hmac_end(Hmac &m, uint8_t *out)
{
    uint8_t inner[64];
    finish(m.in, inner);
    const uint32_t alg = m.in.alg, B = blk_bytes(alg);
    Hash o;
    hinit(o, alg);
    update(o, m.k0, m.klen, 0x5c);
    update_fill(o, 0x5c, B - m.klen);
    update(o, inner, out_bytes(alg));
    finish(o, out);
}

/* HKDF-Expand (RFC 5869 2.3) with info = info1 || info2:
 * T(i) = HMAC(PRK, T(i-1) || info || i), OKM = first L bytes of T(1)||T(2)... */
__device__ void hkdf_expand(uint32_t alg, const uint8_t *prk, uint32_t prk_len, const uint8_t *info1,
                            uint32_t len1, const uint8_t *info2, uint32_t len2, uint8_t *out, uint32_t out_len)
{
    const uint32_t H = out_bytes(alg);
    uint8_t t[64];
    uint32_t done = 0;
    for (uint32_t i = 1; done < out_len; i++) {
        Hmac m;
        hmac_start(m, alg, prk, prk_len);
        if (i > 1) update(m.in, t, H);
        update(m.in, info1, len1);
        update(m.in, info2, len2);
        const uint8_t ctr = (uint8_t) i;
        update(m.in, &ctr, 1);
        hmac_end(m, t);
        const uint32_t take = out_len - done < H ? out_len - done : H;
        for (uint32_t j = 0; j < take; j++) out[done + j] = t[j];
        done += take;
    }
}

/* TLS 1.2 PRF (RFC 5246 5, tls_prf_generic ssl_tls.c:6099) with seed = label || random:
 * A(0) = seed, A(i) = HMAC(secret, A(i-1)), out = HMAC(secret, A(1) || seed) || HMAC(secret, A(2) || seed) ... */
__device__ void tls_prf(uint32_t alg, const uint8_t *secret, uint32_t slen, const uint8_t *label, uint32_t llen,
                        const uint8_t *rnd, uint32_t rlen, uint8_t *out, uint32_t out_len)
{
    const uint32_t H = out_bytes(alg);
    uint8_t a[48], t[48];
    {
        Hmac m;
        hmac_start(m, alg, secret, slen);
        update(m.in, label, llen);
        update(m.in, rnd, rlen);
        hmac_end(m, a);
    }
    uint32_t done = 0;
    while (done < out_len) {
        Hmac m;
        hmac_start(m, alg, secret, slen);
        update(m.in, a, H);
        update(m.in, label, llen);
        update(m.in, rnd, rlen);
        hmac_end(m, t);
        const uint32_t take = out_len - done < H ? out_len - done : H;
        for (uint32_t j = 0; j < take; j++) out[done + j] = t[j];
        done += take;
        if (done < out_len) {
            Hmac n;
            hmac_start(n, alg, secret, slen);
            update(n.in, a, H);
            hmac_end(n, a);
        }
    }
}

/* ---------------- kernels ---------------------------------------------- */
enum { OP_HASH = 0, OP_HMAC = 1, OP_EXPAND = 2, OP_PRF = 3 };

struct Job {
    uint32_t op, alg;
    const uint8_t *key;
    uint32_t key_len;
    const uint8_t *msg;       /* message / info (first part) */
    uint32_t msg_len;
    const uint8_t *msg2;      /* info, second part (a context computed on the device) */
    uint32_t msg2_len;
    uint8_t *out;
    uint32_t out_len;
};

__global__ void __launch_bounds__(64) kdf_job_kernel(const Job *jobs, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Job j = jobs[i];
    if (j.op == OP_HASH) {
        Hash h;
        hinit(h, j.alg);
        update(h, j.msg, j.msg_len);
        update(h, j.msg2, j.msg2_len);
        finish(h, j.out);
    } else if (j.op == OP_HMAC) {
        Hmac m;
        hmac_start(m, j.alg, j.key, j.key_len);
        update(m.in, j.msg, j.msg_len);
        update(m.in, j.msg2, j.msg2_len);
        hmac_end(m, j.out);
    } else if (j.op == OP_PRF) {
        tls_prf(j.alg, j.key, j.key_len, j.msg, j.msg_len, j.msg2, j.msg2_len, j.out, j.out_len);
    } else {
        hkdf_expand(j.alg, j.key, j.key_len, j.msg, j.msg_len, j.msg2, j.msg2_len, j.out, j.out_len);
    }
}

/* Batch traffic-key derivation: one thread per connection direction.
 * infos = HkdfLabel("traffic upd", "", H) || HkdfLabel("key", "", key_len)
 *         || HkdfLabel("iv", "", 12), encoded on the host (same for all). */
struct DeriveArgs {
    tlsrec_tls13_secret *secrets;
    tlsrec_key_material *out;
    uint8_t infos[96];        /* the three encoded HkdfLabels, by value (no host staging buffer) */
    uint32_t len_upd, len_key, len_iv;
    uint32_t count, alg, cipher, key_len, update;
};

__global__ void __launch_bounds__(64) tls13_derive_kernel(DeriveArgs a)
{
    /* the encoded labels (kernel argument) staged once per workgroup */
    __shared__ uint8_t infos[96];
    for (int k = threadIdx.x; k < 96; k += blockDim.x) infos[k] = a.infos[k];
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint32_t H = out_bytes(a.alg);
    uint8_t s[48];
    for (uint32_t k = 0; k < H; k++) s[k] = a.secrets[i].secret[k];
    if (a.update) {
        /* RFC 8446 7.2: secret_N+1 = HKDF-Expand-Label(secret_N, "traffic upd", "", H) */
        uint8_t nx[48];
        hkdf_expand(a.alg, s, H, infos, a.len_upd, nullptr, 0, nx, H);
        for (uint32_t k = 0; k < H; k++) {
            s[k] = nx[k];
            a.secrets[i].secret[k] = nx[k];
        }
    }
    tlsrec_key_material km;
    uint8_t *raw = (uint8_t *) &km;
    for (int k = 0; k < 64; k++) raw[k] = 0;
    km.cipher = (uint8_t) a.cipher;
    km.tls_minor = 4;
    km.fixed_ivlen = 12;      /* TLS 1.3: fixed_ivlen = ivlen = 12, ssl_tls13_keys.c:985-998 */
    km.taglen = (uint8_t) tlsrec_cipher_taglen((int) a.cipher);
    /* ssl_tls13_make_traffic_key, ssl_tls13_keys.c:219-246 */
    hkdf_expand(a.alg, s, H, infos + a.len_upd, a.len_key, nullptr, 0, km.key, a.key_len);
    hkdf_expand(a.alg, s, H, infos + a.len_upd + a.len_key, a.len_iv, nullptr, 0, km.iv, 12);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + i);
    const uint4 *src = reinterpret_cast<const uint4 *>(&km);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = src[k];
}

/* ---------------- TLS 1.2 batch key expansion ---------------------------
 * PRF(master, "key expansion", server_random || client_random) for one
 * connection per lane.  Every shape is fixed (48-byte key, 77-byte seed, at
 * most 88 bytes out for an AEAD suite and 160 for a CBC + HMAC one), so
 * nothing here goes through Hash / put(): the message
 * blocks are assembled as big-endian words with their padding and length
 * words as constants, the compression works on a 16-word window and 8 state
 * words held in registers, and the two HMAC midstates (key ^ ipad, key ^
 * opad) are computed once and reused by every HMAC of the chain.
 *
 * Compressions per connection, n = ceil(out_len / H):
 *   SHA-256: 2 midstates, A(1) 3 (seed 77 B: two inner blocks + outer),
 *            A(i>1) 2, each output block 3 (A || seed = 109 B)  -> 5n + 3
 *   SHA-384: 2 midstates, A(i) 2, each output block 3 (A || seed = 125 B:
 *            the padding spills into a second, constant block)  -> 5n + 2 */
/* a big-endian 32-bit word of device memory, by one aligned load or by bytes */
__device__ __forceinline__ uint32_t load_be32(const uint8_t *p, bool aligned)
{
    if (aligned) return __builtin_bswap32(*reinterpret_cast<const uint32_t *>(p));
    return ((uint32_t) p[0] << 24) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 8) | p[3];
}

/* The 77-byte seed "key expansion" || randbytes as big-endian words: the
 * 13-byte label leaves the random words one byte off, S[3 + k] =
 * R[k-1] << 24 | R[k] >> 8; S[19] holds the last byte and the 0x80 that
 * follows the seed wherever it ends a message. */
__device__ __forceinline__ void tls12_seed_words(const uint32_t (&R)[16], uint32_t (&S)[20])
{
    S[0] = 0x6b657920u;      /* "key " */
    S[1] = 0x65787061u;      /* "expa" */
    S[2] = 0x6e73696fu;      /* "nsio" */
    S[3] = 0x6e000000u | (R[0] >> 8);   /* "n" */
#pragma unroll
    for (int k = 1; k < 16; k++) S[3 + k] = (R[k - 1] << 24) | (R[k] >> 8);
    S[19] = (R[15] << 24) | 0x00800000u;
}

/* P_SHA256: KB (KBW words, the key block of the caller's shape) receives 8
 * words per iteration, ITERS = ceil(out_len / 32) */
template <int ITERS, int KBW>
__device__ __forceinline__ void tls12_expand_sha256(const uint32_t (&M)[12], const uint32_t (&R)[16],
                                                    uint32_t (&KB)[KBW])
{
    static_assert(ITERS * 8 <= KBW, "key block holds every iteration's digest");
    const uint32_t iv[8] = { 0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                             0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u };
    const uint32_t HMAC_LEN = (64 + 32) * 8;     /* bits of key block || 32-byte digest */
    uint32_t S[20], w[16], ip[8], op[8], st[8], A[8];
    tls12_seed_words(R, S);
    /* midstates: one block of master ^ pad, master zero-padded to 64 bytes (RFC 2104) */
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = (j < 12 ? M[j] : 0u) ^ 0x36363636u;
#pragma unroll
    for (int j = 0; j < 8; j++) ip[j] = iv[j];
    sha_compress<S256>(ip, w);
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = (j < 12 ? M[j] : 0u) ^ 0x5c5c5c5cu;
#pragma unroll
    for (int j = 0; j < 8; j++) op[j] = iv[j];
    sha_compress<S256>(op, w);
    /* outer hash of an HMAC: opad midstate over the 32-byte inner digest in st */
    auto outer = [&](uint32_t (&dst)[8]) {
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = st[j];
        w[8] = 0x80000000u;
#pragma unroll
        for (int j = 9; j < 15; j++) w[j] = 0;
        w[15] = HMAC_LEN;
#pragma unroll
        for (int j = 0; j < 8; j++) dst[j] = op[j];
        sha_compress<S256>(dst, w);
    };
#pragma unroll
    for (int j = 0; j < 8; j++) A[j] = 0;
#pragma unroll 1
    for (int it = 0; it < ITERS; it++) {
        /* A(it + 1) = HMAC(A(it)); A(0) is the seed, whose 77 bytes take a second block */
        const bool first = it == 0;
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = first ? S[j] : A[j];
        w[8] = first ? S[8] : 0x80000000u;
#pragma unroll
        for (int j = 9; j < 15; j++) w[j] = first ? S[j] : 0u;
        w[15] = first ? S[15] : HMAC_LEN;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        sha_compress<S256>(st, w);
        if (first) {
            w[0] = S[16]; w[1] = S[17]; w[2] = S[18]; w[3] = S[19];
#pragma unroll
            for (int j = 4; j < 15; j++) w[j] = 0;
            w[15] = (64 + 77) * 8;
            sha_compress<S256>(st, w);
        }
        outer(A);
        /* output block = HMAC(A || seed): 109 bytes, 64 + 45 */
#pragma unroll
        for (int j = 0; j < 8; j++) { w[j] = A[j]; w[8 + j] = S[j]; }
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        sha_compress<S256>(st, w);
#pragma unroll
        for (int j = 0; j < 12; j++) w[j] = S[8 + j];
        w[12] = 0; w[13] = 0; w[14] = 0;
        w[15] = (64 + 109) * 8;
        sha_compress<S256>(st, w);
        uint32_t D[8];
        outer(D);
#pragma unroll
        for (int q = 0; q < ITERS; q++) {
            if (it == q) {
#pragma unroll
                for (int j = 0; j < 8; j++) KB[8 * q + j] = D[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) D[j] = 0;
    }
    /* the reference zeroizes keyblk and the PSA operation; nothing of the chain stays behind */
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; st[j] = 0; A[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int j = 0; j < 20; j++) S[j] = 0;
}

/* P_SHA384 (SHA-512 compression, 128-byte blocks, 48-byte digests): KB
 * receives 12 words per iteration, ITERS = ceil(out_len / 48) */
template <int ITERS, int KBW>
__device__ __forceinline__ void tls12_expand_sha384(const uint32_t (&M)[12], const uint32_t (&R)[16],
                                                    uint32_t (&KB)[KBW])
{
    static_assert(ITERS * 12 <= KBW, "key block holds every iteration's digest");
    const uint64_t iv[8] = { 0xcbbb9d5dc1059ed8ULL, 0x629a292a367cd507ULL, 0x9159015a3070dd17ULL,
                             0x152fecd8f70e5939ULL, 0x67332667ffc00b31ULL, 0x8eb44a8768581511ULL,
                             0xdb0c2e0d64f98fa7ULL, 0x47b5481dbefa4fa4ULL };
    const uint64_t HMAC_LEN = (128 + 48) * 8;
    uint32_t S[20];
    uint64_t T[10], w[16], ip[8], op[8], st[8], A[6];
    tls12_seed_words(R, S);
#pragma unroll
    for (int j = 0; j < 10; j++) T[j] = ((uint64_t) S[2 * j] << 32) | S[2 * j + 1];   /* T[9]: 5 seed bytes, 0x80 */
#pragma unroll
    for (int j = 0; j < 16; j++)
        w[j] = (j < 6 ? (((uint64_t) M[2 * j] << 32) | M[2 * j + 1]) : 0ULL) ^ 0x3636363636363636ULL;
#pragma unroll
    for (int j = 0; j < 8; j++) ip[j] = iv[j];
    sha_compress<S512>(ip, w);
#pragma unroll
    for (int j = 0; j < 16; j++)
        w[j] = (j < 6 ? (((uint64_t) M[2 * j] << 32) | M[2 * j + 1]) : 0ULL) ^ 0x5c5c5c5c5c5c5c5cULL;
#pragma unroll
    for (int j = 0; j < 8; j++) op[j] = iv[j];
    sha_compress<S512>(op, w);
    /* outer hash: opad midstate over the first 48 bytes of st; the first 6 words of the result */
    auto outer = [&](uint64_t (&dst)[6]) {
        uint64_t o[8];
#pragma unroll
        for (int j = 0; j < 6; j++) w[j] = st[j];
        w[6] = 0x8000000000000000ULL;
#pragma unroll
        for (int j = 7; j < 15; j++) w[j] = 0;
        w[15] = HMAC_LEN;
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = op[j];
        sha_compress<S512>(o, w);
#pragma unroll
        for (int j = 0; j < 6; j++) dst[j] = o[j];
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = 0;
    };
#pragma unroll
    for (int j = 0; j < 6; j++) A[j] = 0;
#pragma unroll 1
    for (int it = 0; it < ITERS; it++) {
        /* A(it + 1) = HMAC(A(it)): the 77-byte seed or a 48-byte digest, one block either way */
        const bool first = it == 0;
#pragma unroll
        for (int j = 0; j < 6; j++) w[j] = first ? T[j] : A[j];
        w[6] = first ? T[6] : 0x8000000000000000ULL;
#pragma unroll
        for (int j = 7; j < 10; j++) w[j] = first ? T[j] : 0ULL;
#pragma unroll
        for (int j = 10; j < 15; j++) w[j] = 0;
        w[15] = first ? (uint64_t) ((128 + 77) * 8) : HMAC_LEN;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        sha_compress<S512>(st, w);
        outer(A);
        /* output block = HMAC(A || seed): 125 bytes fill the block up to its last
         * 3 bytes, so the 0x80 is in T[9] and the length goes to a second block */
#pragma unroll
        for (int j = 0; j < 6; j++) w[j] = A[j];
#pragma unroll
        for (int j = 0; j < 10; j++) w[6 + j] = T[j];
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        sha_compress<S512>(st, w);
#pragma unroll
        for (int j = 0; j < 15; j++) w[j] = 0;
        w[15] = (128 + 125) * 8;
        sha_compress<S512>(st, w);
        uint64_t D[6];
        outer(D);
#pragma unroll
        for (int q = 0; q < ITERS; q++) {
            if (it == q) {
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    KB[12 * q + 2 * j] = (uint32_t) (D[j] >> 32);
                    KB[12 * q + 2 * j + 1] = (uint32_t) D[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 6; j++) D[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; st[j] = 0; }
#pragma unroll
    for (int j = 0; j < 6; j++) A[j] = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int j = 0; j < 10; j++) T[j] = 0;
#pragma unroll
    for (int j = 0; j < 20; j++) S[j] = 0;
}

/* One connection's master secret and random bytes as big-endian words: seven
 * 16-byte loads, or bytes when the array is not 16-byte aligned. */
__device__ __forceinline__ void tls12_load_conn(const tlsrec_tls12_conn *conn, bool aligned, uint32_t (&M)[12],
                                                uint32_t (&R)[16])
{
    const uint8_t *c = reinterpret_cast<const uint8_t *>(conn);
    if (aligned) {
        const uint4 *q = reinterpret_cast<const uint4 *>(c);
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const uint4 v = q[k];
            const uint32_t x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int n = 4 * k + j;
                if (n < 12) M[n] = __builtin_bswap32(x[j]);
                else R[n - 12] = __builtin_bswap32(x[j]);
            }
        }
    } else {
#pragma unroll
        for (int n = 0; n < 12; n++) M[n] = load_be32(c + 4 * n, false);
#pragma unroll
        for (int n = 0; n < 16; n++) R[n] = load_be32(c + 48 + 4 * n, false);
    }
}

struct Tls12Args {
    const tlsrec_tls12_conn *conns;
    tlsrec_key_material *out;     /* staging area of slot `first`: 2 records per connection */
    uint32_t count, cipher, taglen, aligned;
};

/* One lane per connection; KL / IVL = the cipher's key length and TLS 1.2
 * fixed_ivlen, so the split of the key block (ssl_tls.c:7858-7892) indexes
 * registers with constants. */
template <int ALG, int KL, int IVL> __global__ void __launch_bounds__(64) tls12_derive_kernel(Tls12Args a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    constexpr int OUT = 2 * KL + 2 * IVL, H = ALG == H_SHA384 ? 48 : 32, ITERS = (OUT + H - 1) / H;
    static_assert(ITERS * H <= 96 && KL % 4 == 0 && IVL % 4 == 0, "key block shape");
    uint32_t M[12], R[16], KB[24];
    tls12_load_conn(a.conns + i, a.aligned != 0, M, R);
#pragma unroll
    for (int j = 0; j < 24; j++) KB[j] = 0;
    if constexpr (ALG == H_SHA384) tls12_expand_sha384<ITERS>(M, R, KB);
    else tls12_expand_sha256<ITERS>(M, R, KB);
    /* tlsrec_key_material: cipher, tls_minor 3, fixed_ivlen, taglen | granularity 0, reserved |
     * iv[16] | key[32]; client_write first, then server_write */
    const uint32_t head = a.cipher | (3u << 8) | ((uint32_t) IVL << 16) | (a.taglen << 24);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + 2 * (size_t) i);
#pragma unroll
    for (int side = 0; side < 2; side++) {
        uint32_t km[16];
        km[0] = head;
#pragma unroll
        for (int j = 1; j < 16; j++) km[j] = 0;
#pragma unroll
        for (int j = 0; j < IVL / 4; j++) km[4 + j] = __builtin_bswap32(KB[2 * KL / 4 + side * (IVL / 4) + j]);
#pragma unroll
        for (int j = 0; j < KL / 4; j++) km[8 + j] = __builtin_bswap32(KB[side * (KL / 4) + j]);
#pragma unroll
        for (int k = 0; k < 4; k++) dst[4 * side + k] = make_uint4(km[4 * k], km[4 * k + 1], km[4 * k + 2], km[4 * k + 3]);
#pragma unroll
        for (int j = 0; j < 16; j++) km[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 24; j++) KB[j] = 0;
#pragma unroll
    for (int j = 0; j < 12; j++) M[j] = 0;
}

struct Tls12CbcArgs {
    const tlsrec_tls12_conn *conns;
    tlsrec_cbc_key_material *out;     /* CBC staging area of slot `first`: 2 records per connection */
    uint32_t count, head, aligned;    /* head: cipher | tls_minor 3 | mac | etm, the first word of a record */
};

/* The CBC + HMAC suites: the key block is client_mac | server_mac | client_key
 * | server_key (ssl_tls.c:7858-7886, mac_key_len != 0; TLS 1.2 carries the CBC
 * IV in each record, so no IV is derived), 72 to 160 bytes = 3 to 5 P_SHA256 or
 * 2 to 4 P_SHA384 iterations.  One lane per connection as above; KL / ML = the
 * key and MAC key lengths, all multiples of 4 bytes, so the split indexes
 * registers with constants.  Each side is one tlsrec_cbc_key_material (128
 * bytes: head, 44 reserved bytes, key at byte 48, mac_key at byte 80). */
template <int ALG, int KL, int ML> __global__ void __launch_bounds__(64) tls12_derive_cbc_kernel(Tls12CbcArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    constexpr int OUT = 2 * ML + 2 * KL, H = ALG == H_SHA384 ? 48 : 32, ITERS = (OUT + H - 1) / H;
    constexpr int KBW = ITERS * H / 4;
    static_assert(KL % 4 == 0 && KL <= 32 && ML % 4 == 0 && ML <= 48, "key block shape");
    static_assert(sizeof(tlsrec_cbc_key_material) == 128 && offsetof(tlsrec_cbc_key_material, key) == 48 &&
                  offsetof(tlsrec_cbc_key_material, mac_key) == 80, "tlsrec_cbc_key_material layout");
    uint32_t M[12], R[16], KB[KBW];
    tls12_load_conn(a.conns + i, a.aligned != 0, M, R);
#pragma unroll
    for (int j = 0; j < KBW; j++) KB[j] = 0;
    if constexpr (ALG == H_SHA384) tls12_expand_sha384<ITERS>(M, R, KB);
    else tls12_expand_sha256<ITERS>(M, R, KB);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + 2 * (size_t) i);
#pragma unroll
    for (int side = 0; side < 2; side++) {
        uint32_t km[32];
        km[0] = a.head;
#pragma unroll
        for (int j = 1; j < 32; j++) km[j] = 0;
#pragma unroll
        for (int j = 0; j < KL / 4; j++) km[12 + j] = __builtin_bswap32(KB[2 * ML / 4 + side * (KL / 4) + j]);
#pragma unroll
        for (int j = 0; j < ML / 4; j++) km[20 + j] = __builtin_bswap32(KB[side * (ML / 4) + j]);
#pragma unroll
        for (int k = 0; k < 8; k++) dst[8 * side + k] = make_uint4(km[4 * k], km[4 * k + 1], km[4 * k + 2], km[4 * k + 3]);
#pragma unroll
        for (int j = 0; j < 32; j++) km[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < KBW; j++) KB[j] = 0;
#pragma unroll
    for (int j = 0; j < 12; j++) M[j] = 0;
}

/* ---------------- TLS 1.3 ladder, batch ----------------------------------
 * Early Secret -> Handshake Secret -> handshake traffic keys and Finished
 * keys -> Master Secret -> application traffic keys (RFC 8446 7.1; the helpers
 * of ssl_tls13_keys.c:421-650 and ssl_tls13_calc_finished_core :697), one
 * connection per lane.  As in the TLS 1.2 kernels nothing goes through Hash /
 * put(): every message here is a single inner block whose words are put
 * together with constant indices -- an HkdfLabel with a label of at most 12
 * characters and a context of H bytes, || 0x01, is at most 55 bytes (SHA-256)
 * or 71 (SHA-384) -- except the Extract over a 56- or 66-byte shared secret
 * under SHA-256, which takes a second one.  The HMAC midstates of a secret are
 * computed once and serve every Expand under it; the midstates of the zero
 * salt, Hash("") and, for a connection without a PSK, the midstates of
 * Derive-Secret(Early Secret, "derived", "") are the same for every connection
 * and arrive as kernel arguments (LadderConsts, scalar registers).
 *
 * Messages are addressed in 32-bit big-endian cells: 16 to a SHA-256 block, 32
 * to a SHA-512 one. */
struct L256 {
    typedef S256 S;
    typedef uint32_t W;
    enum { HW = 8, HC = 8, HB = 32, BB = 64, LENB = 8 };
    static __device__ __forceinline__ W iv(int j)
    {
        const W t[8] = { 0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                         0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u };
        return t[j];
    }
};
struct L384 {
    typedef S512 S;
    typedef uint64_t W;
    enum { HW = 6, HC = 12, HB = 48, BB = 128, LENB = 16 };
    static __device__ __forceinline__ W iv(int j)
    {
        const W t[8] = { 0xcbbb9d5dc1059ed8ULL, 0x629a292a367cd507ULL, 0x9159015a3070dd17ULL,
                         0x152fecd8f70e5939ULL, 0x67332667ffc00b31ULL, 0x8eb44a8768581511ULL,
                         0xdb0c2e0d64f98fa7ULL, 0x47b5481dbefa4fa4ULL };
        return t[j];
    }
};

/* the constants of one hash (values in ladder_consts() on the host side) */
template <class T> struct LadderConsts {
    typename T::W zero_ip[8], zero_op[8];   /* HMAC midstates of a salt of H zero bytes */
    typename T::W d0_ip[8], d0_op[8];       /* ... of Derive-Secret(Extract(0, 0), "derived", "") */
    typename T::W empty[T::HW];             /* Hash("") */
};

/* An HkdfLabel up to and including its context-length byte (ssl_tls13_keys.c:98-136)
 * as big-endian cells, zero-padded: 10 + label_len <= 22 bytes.  Encoded on the host. */
struct LabelW { uint32_t c[6]; };

/* cell i of a block / of a digest; i is a constant wherever these are used */
template <class T> __device__ __forceinline__ void or_cell(typename T::W (&w)[16], int i, uint32_t v)
{
    if constexpr (sizeof(typename T::W) == 4) w[i] |= v;
    else w[i >> 1] |= (uint64_t) v << ((i & 1) ? 0 : 32);
}
template <class T, int N> __device__ __forceinline__ uint32_t cell(const typename T::W (&x)[N], int i)
{
    if constexpr (sizeof(typename T::W) == 4) return x[i];
    else return (i & 1) ? (uint32_t) x[i >> 1] : (uint32_t) (x[i >> 1] >> 32);
}
/* the 4 bytes of v at byte position p of the block */
template <class T> __device__ __forceinline__ void or_cell_at(typename T::W (&w)[16], int p, uint32_t v)
{
    const int i = p >> 2, r = p & 3;
    or_cell<T>(w, i, r ? v >> (8 * r) : v);
    if (r) or_cell<T>(w, i + 1, v << (32 - 8 * r));
}
template <class T> __device__ __forceinline__ void or_byte_at(typename T::W (&w)[16], int p, uint32_t b)
{
    or_cell<T>(w, p >> 2, b << (24 - 8 * (p & 3)));
}

/* the two midstates of HMAC under an H-byte key: 2 compressions */
template <class T>
__device__ __forceinline__ void hmac_mid(const typename T::W (&key)[T::HW], typename T::W (&ip)[8], typename T::W (&op)[8])
{
    typedef typename T::W W;
    W w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = (j < T::HW ? key[j] : (W) 0) ^ (W) 0x3636363636363636ULL;
#pragma unroll
    for (int j = 0; j < 8; j++) ip[j] = T::iv(j);
    sha_compress<typename T::S>(ip, w);
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = (j < T::HW ? key[j] : (W) 0) ^ (W) 0x5c5c5c5c5c5c5c5cULL;
#pragma unroll
    for (int j = 0; j < 8; j++) op[j] = T::iv(j);
    sha_compress<typename T::S>(op, w);
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* the outer hash: opad midstate over the inner digest in st (consumed): 1 compression */
template <class T>
__device__ __forceinline__ void hmac_outer(const typename T::W (&op)[8], typename T::W (&st)[8], typename T::W (&out)[T::HW])
{
    typedef typename T::W W;
    W w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = j < T::HW ? st[j] : (W) 0;
    w[T::HW] = (W) 0x80 << (8 * sizeof(W) - 8);
    w[15] = (T::BB + T::HB) * 8;
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = op[j];
    sha_compress<typename T::S>(st, w);
#pragma unroll
    for (int j = 0; j < T::HW; j++) out[j] = st[j];
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* HMAC of a message that is the one inner block w (padding and length in place; consumed): 2 compressions */
template <class T>
__device__ __forceinline__ void hmac_block(const typename T::W (&ip)[8], const typename T::W (&op)[8],
                                           typename T::W (&w)[16], typename T::W (&out)[T::HW])
{
    typename T::W st[8];
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = ip[j];
    sha_compress<typename T::S>(st, w);
    hmac_outer<T>(op, st, out);
}

/* the inner block of an H-byte message (an Extract over a secret or over H zero bytes, a Finished MAC) */
template <class T> __device__ __forceinline__ void digest_block(typename T::W (&w)[16], const typename T::W (&x)[T::HW])
{
    typedef typename T::W W;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = j < T::HW ? x[j] : (W) 0;
    w[T::HW] = (W) 0x80 << (8 * sizeof(W) - 8);
    w[15] = (T::BB + T::HB) * 8;
}

/* the inner block of HKDF-Expand-Label's one HMAC: HkdfLabel (OFF bytes up to
 * the context, then the H-byte context if CTX) || 0x01 */
template <class T, int OFF, bool CTX>
__device__ __forceinline__ void label_block(typename T::W (&w)[16], const LabelW &lb, const typename T::W (&ctx)[T::HW])
{
    constexpr int END = OFF + (CTX ? (int) T::HB : 0);
    static_assert(OFF <= 22 && END + 2 + T::LENB <= T::BB, "HkdfLabel || 0x01 pads into one block");
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int c = 0; c < (OFF + 3) / 4; c++) or_cell<T>(w, c, lb.c[c]);
    if constexpr (CTX) {
#pragma unroll
        for (int c = 0; c < T::HC; c++) or_cell_at<T>(w, OFF + 4 * c, cell<T, T::HW>(ctx, c));
    }
    or_byte_at<T>(w, END, 0x01);
    or_byte_at<T>(w, END + 1, 0x80);
    w[15] = (T::BB + END + 1) * 8;
}

/* block `blk` of a message of n bytes (n wave-uniform, n + 1 + LENB <= 2 * BB)
 * held in the cells m[]: bytes past n are masked off, 0x80 follows the message
 * and the length closes the last block */
template <class T, int NC>
__device__ __forceinline__ void msg_block(typename T::W (&w)[16], const uint32_t (&m)[NC], uint32_t n, int blk)
{
    constexpr int CPB = T::BB / 4;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int c = 0; c < CPB; c++) {
        const int g = blk * CPB + c;              /* blk is 0 or 1 at every call: g is a constant */
        const int rem = (int) n - 4 * g;
        const uint32_t v = g < NC ? m[g] : 0u;
        uint32_t x;
        if (rem >= 4) x = v;
        else if (rem > 0) x = (v & ~(0xffffffffu >> (8 * rem))) | (0x80u << (24 - 8 * rem));
        else x = rem == 0 ? 0x80000000u : 0u;
        or_cell<T>(w, c, x);
    }
    if ((int) n + 1 + (int) T::LENB <= (blk + 1) * (int) T::BB) w[15] = (typename T::W) ((T::BB + n) * 8);
}

/* NC cells from device memory: 16-byte loads, or bytes when the array is not 16-byte aligned */
template <int NC> __device__ __forceinline__ void load_cells(const uint8_t *p, bool aligned, uint32_t (&m)[NC])
{
    if (aligned) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
        for (int k = 0; k < (NC + 3) / 4; k++) {
            const uint4 v = q[k];
            const uint32_t x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (4 * k + j < NC) m[4 * k + j] = __builtin_bswap32(x[j]);
        }
    } else {
#pragma unroll
        for (int n = 0; n < NC; n++) m[n] = load_be32(p + 4 * n, false);
    }
}

template <class T> __device__ __forceinline__ void load_digest(const uint8_t *p, bool aligned, typename T::W (&x)[T::HW])
{
    uint32_t m[T::HC];
    load_cells<T::HC>(p, aligned, m);
#pragma unroll
    for (int j = 0; j < T::HW; j++) {
        if constexpr (sizeof(typename T::W) == 4) x[j] = m[j];
        else x[j] = ((uint64_t) m[2 * j] << 32) | m[2 * j + 1];
    }
#pragma unroll
    for (int j = 0; j < T::HC; j++) m[j] = 0;
}

/* a tlsrec_tls13_secret: H bytes of x, the rest zero; three 16-byte stores, or bytes */
template <class T> __device__ __forceinline__ void store_secret(tlsrec_tls13_secret *dst, bool aligned, const typename T::W (&x)[T::HW])
{
    uint32_t m[12];
#pragma unroll
    for (int c = 0; c < 12; c++) m[c] = c < T::HC ? __builtin_bswap32(cell<T, T::HW>(x, c)) : 0u;
    if (aligned) {
        uint4 *q = reinterpret_cast<uint4 *>(dst);
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = make_uint4(m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]);
    } else {
        uint8_t *b = dst->secret;
#pragma unroll
        for (int c = 0; c < 12; c++) {
            b[4 * c] = (uint8_t) m[c]; b[4 * c + 1] = (uint8_t) (m[c] >> 8);
            b[4 * c + 2] = (uint8_t) (m[c] >> 16); b[4 * c + 3] = (uint8_t) (m[c] >> 24);
        }
    }
#pragma unroll
    for (int c = 0; c < 12; c++) m[c] = 0;
}

/* the labels of one stage, each with its Hash.length / key length / 12 as the
 * output length and the context length it is used with */
struct LadderLabels { LabelW derived, c_traffic, s_traffic, extra, key, iv, fin; };
enum { OFF_DERIVED = 17, OFF_TRAFFIC = 22, OFF_EXP_MASTER = 20, OFF_KEY = 13, OFF_IV = 12, OFF_FINISHED = 18 };

/* One direction under its traffic secret ts: write_key, write_iv
 * (ssl_tls13_make_traffic_key, ssl_tls13_keys.c:219-246) as a
 * tlsrec_key_material, and the Finished key if fin != NULL.  2 + 4 (+ 2)
 * compressions. */
template <class T>
__device__ __forceinline__ void traffic_side(const typename T::W (&ts)[T::HW], const LadderLabels &lb, uint32_t head,
                                             uint32_t key_cells, tlsrec_key_material *km_dst, tlsrec_tls13_secret *fin,
                                             bool fin_aligned)
{
    typedef typename T::W W;
    W ip[8], op[8], w[16], K[T::HW], V[T::HW];
    hmac_mid<T>(ts, ip, op);
    label_block<T, OFF_KEY, false>(w, lb.key, K);
    hmac_block<T>(ip, op, w, K);
    label_block<T, OFF_IV, false>(w, lb.iv, V);
    hmac_block<T>(ip, op, w, V);
    uint32_t km[16];
    km[0] = head;
#pragma unroll
    for (int j = 1; j < 16; j++) km[j] = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) km[4 + j] = __builtin_bswap32(cell<T, T::HW>(V, j));
#pragma unroll
    for (int j = 0; j < 8; j++) km[8 + j] = (uint32_t) j < key_cells ? __builtin_bswap32(cell<T, T::HW>(K, j)) : 0u;
    uint4 *dst = reinterpret_cast<uint4 *>(km_dst);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = make_uint4(km[4 * k], km[4 * k + 1], km[4 * k + 2], km[4 * k + 3]);
    if (fin) {
        label_block<T, OFF_FINISHED, false>(w, lb.fin, K);
        hmac_block<T>(ip, op, w, K);
        store_secret<T>(fin, fin_aligned, K);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) km[j] = 0;
#pragma unroll
    for (int j = 0; j < T::HW; j++) { K[j] = 0; V[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
}

enum { AL_CONNS = 1, AL_TRAFFIC = 2, AL_AUX = 4, AL_MASTER = 8, AL_TRANSCRIPT = 16 };

template <class T> struct Tls13HsArgs {
    const tlsrec_tls13_hs_conn *conns;
    tlsrec_key_material *out;             /* staging area of slot `first`: 2 records per connection */
    tlsrec_tls13_secret *hs_traffic, *finished, *master;
    uint32_t count, head, key_cells, psk_len, shared_len, aligned;
    LadderConsts<T> k;
    LadderLabels lb;
};

/* Compressions per connection: no PSK 0, a PSK 8 (Extract 2,
 * midstates 2, "derived" 2, midstates 2); Extract over the shared secret 2 (3
 * for 56 / 66 bytes under SHA-256); midstates 2; two traffic secrets 4;
 * "derived" 2, midstates 2, Master Secret 2; each direction 2 + key 2 + iv 2 +
 * finished 2: 30 / 38 with both Finished keys, 26 / 34 without. */
template <class T> __global__ void __launch_bounds__(64) tls13_hs_kernel(Tls13HsArgs<T> a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint8_t *conn = reinterpret_cast<const uint8_t *>(a.conns + i);
    const bool cal = (a.aligned & AL_CONNS) != 0;
    W ip[8], op[8], w[16], x[T::HW];
    if (a.psk_len) {
        /* Early Secret = Extract(0, PSK); then the salt of the next Extract */
        uint32_t P[12];
        load_cells<12>(conn, cal, P);
        msg_block<T, 12>(w, P, a.psk_len, 0);
        hmac_block<T>(a.k.zero_ip, a.k.zero_op, w, x);
        hmac_mid<T>(x, ip, op);
        label_block<T, OFF_DERIVED, true>(w, a.lb.derived, a.k.empty);
        hmac_block<T>(ip, op, w, x);
        hmac_mid<T>(x, ip, op);
#pragma unroll
        for (int j = 0; j < 12; j++) P[j] = 0;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) { ip[j] = a.k.d0_ip[j]; op[j] = a.k.d0_op[j]; }
    }
    /* Handshake Secret = Extract(., shared), H zero bytes for psk_ke */
    {
        W st[8];
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        if (a.shared_len) {
            uint32_t Sh[20];
            load_cells<20>(conn + 48, cal, Sh);
            msg_block<T, 20>(w, Sh, a.shared_len, 0);
            sha_compress<typename T::S>(st, w);
            if (a.shared_len + 1 + T::LENB > T::BB) {
                msg_block<T, 20>(w, Sh, a.shared_len, 1);
                sha_compress<typename T::S>(st, w);
            }
#pragma unroll
            for (int j = 0; j < 20; j++) Sh[j] = 0;
        } else {
#pragma unroll
            for (int j = 0; j < T::HW; j++) x[j] = 0;
            digest_block<T>(w, x);
            sha_compress<typename T::S>(st, w);
        }
        hmac_outer<T>(op, st, x);
    }
    hmac_mid<T>(x, ip, op);
    W tr[T::HW], cs[T::HW], ss[T::HW];
    load_digest<T>(conn + 128, cal, tr);
    label_block<T, OFF_TRAFFIC, true>(w, a.lb.c_traffic, tr);
    hmac_block<T>(ip, op, w, cs);
    label_block<T, OFF_TRAFFIC, true>(w, a.lb.s_traffic, tr);
    hmac_block<T>(ip, op, w, ss);
    /* Master Secret = Extract(Derive-Secret(Handshake Secret, "derived", ""), 0) */
    label_block<T, OFF_DERIVED, true>(w, a.lb.derived, a.k.empty);
    hmac_block<T>(ip, op, w, x);
    hmac_mid<T>(x, ip, op);
#pragma unroll
    for (int j = 0; j < T::HW; j++) x[j] = 0;
    digest_block<T>(w, x);
    hmac_block<T>(ip, op, w, x);
    store_secret<T>(a.master + i, (a.aligned & AL_MASTER) != 0, x);
    store_secret<T>(a.hs_traffic + 2 * (size_t) i, (a.aligned & AL_TRAFFIC) != 0, cs);
    store_secret<T>(a.hs_traffic + 2 * (size_t) i + 1, (a.aligned & AL_TRAFFIC) != 0, ss);
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
#pragma unroll
        for (int j = 0; j < T::HW; j++) x[j] = side ? ss[j] : cs[j];
        traffic_side<T>(x, a.lb, a.head, a.key_cells, a.out + 2 * (size_t) i + side,
                        a.finished ? a.finished + 2 * (size_t) i + side : nullptr, (a.aligned & AL_AUX) != 0);
    }
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; cs[j] = 0; ss[j] = 0; tr[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

template <class T> struct Tls13AppArgs {
    const tlsrec_tls13_secret *master, *transcripts;
    tlsrec_key_material *out;
    tlsrec_tls13_secret *app_traffic, *exporter;
    uint32_t count, head, key_cells, aligned;
    LadderLabels lb;                      /* extra: "exp master" */
};

/* Compressions per connection: midstates 2, two traffic secrets 4, exporter
 * master secret 2, each direction 2 + key 2 + iv 2: 20, 18 without the exporter. */
template <class T> __global__ void __launch_bounds__(64) tls13_app_kernel(Tls13AppArgs<T> a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8], w[16], x[T::HW], tr[T::HW], cs[T::HW], ss[T::HW];
    load_digest<T>(a.master[i].secret, (a.aligned & AL_MASTER) != 0, x);
    load_digest<T>(a.transcripts[i].secret, (a.aligned & AL_TRANSCRIPT) != 0, tr);
    hmac_mid<T>(x, ip, op);
    label_block<T, OFF_TRAFFIC, true>(w, a.lb.c_traffic, tr);
    hmac_block<T>(ip, op, w, cs);
    label_block<T, OFF_TRAFFIC, true>(w, a.lb.s_traffic, tr);
    hmac_block<T>(ip, op, w, ss);
    if (a.exporter) {
        label_block<T, OFF_EXP_MASTER, true>(w, a.lb.extra, tr);
        hmac_block<T>(ip, op, w, x);
        store_secret<T>(a.exporter + i, (a.aligned & AL_AUX) != 0, x);
    }
    store_secret<T>(a.app_traffic + 2 * (size_t) i, (a.aligned & AL_TRAFFIC) != 0, cs);
    store_secret<T>(a.app_traffic + 2 * (size_t) i + 1, (a.aligned & AL_TRAFFIC) != 0, ss);
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
#pragma unroll
        for (int j = 0; j < T::HW; j++) x[j] = side ? ss[j] : cs[j];
        traffic_side<T>(x, a.lb, a.head, a.key_cells, a.out + 2 * (size_t) i + side, nullptr, false);
    }
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; cs[j] = 0; ss[j] = 0; tr[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* out[i] = HMAC(keys[i], msgs[i]) over H-byte messages (verify_data under a
 * Finished key), or with label_len != ~0u Expand-Label(keys[i], label, msgs[i], H)
 * (Derive-Secret with a hashed context): 4 compressions either way. */
struct Tls13MacArgs {
    const tlsrec_tls13_secret *keys, *msgs;
    tlsrec_tls13_secret *out;
    uint32_t count, aligned, label_len;   /* AL_MASTER keys, AL_TRANSCRIPT msgs, AL_AUX out */
    LabelW label;
};
enum : uint32_t { MAC_PLAIN = ~0u };

template <class T> __global__ void __launch_bounds__(64) tls13_mac_kernel(Tls13MacArgs a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8], w[16], x[T::HW], m[T::HW];
    load_digest<T>(a.keys[i].secret, (a.aligned & AL_MASTER) != 0, x);
    load_digest<T>(a.msgs[i].secret, (a.aligned & AL_TRANSCRIPT) != 0, m);
    hmac_mid<T>(x, ip, op);
    /* the label's length only moves the context inside the block: wave-uniform */
    switch (a.label_len) {
        case 0: label_block<T, 10, true>(w, a.label, m); break;
        case 1: label_block<T, 11, true>(w, a.label, m); break;
        case 2: label_block<T, 12, true>(w, a.label, m); break;
        case 3: label_block<T, 13, true>(w, a.label, m); break;
        case 4: label_block<T, 14, true>(w, a.label, m); break;
        case 5: label_block<T, 15, true>(w, a.label, m); break;
        case 6: label_block<T, 16, true>(w, a.label, m); break;
        case 7: label_block<T, 17, true>(w, a.label, m); break;
        case 8: label_block<T, 18, true>(w, a.label, m); break;
        case 9: label_block<T, 19, true>(w, a.label, m); break;
        case 10: label_block<T, 20, true>(w, a.label, m); break;
        case 11: label_block<T, 21, true>(w, a.label, m); break;
        case 12: label_block<T, 22, true>(w, a.label, m); break;
        default: digest_block<T>(w, m); break;
    }
    hmac_block<T>(ip, op, w, x);
    store_secret<T>(a.out + i, (a.aligned & AL_AUX) != 0, x);
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; m[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* ---- a resumed handshake: PSK binder, 0-RTT keys, ticket PSK ---------------
 * An HkdfLabel up to and including its context-length byte is 2 (length) + 1
 * (label length) + 6 ("tls13 ") + the label + 1 bytes, so the context starts
 * at 10 + strlen(label): "res binder" / "ext binder" (10 characters) 20,
 * "c e traffic" (11) 21, "e exp master" (12) 22, "resumption" (10) 20. */
enum { OFF_BINDER = 20, OFF_E_TRAFFIC = 21, OFF_E_EXP_MASTER = 22, OFF_RESUMPTION = 20 };
enum { AL_BINDERS = AL_MASTER, AL_OFFERED = AL_TRANSCRIPT };

template <class T> struct Tls13EarlyArgs {
    const tlsrec_tls13_psk_conn *conns;
    const tlsrec_tls13_secret *offered;   /* with match, or both NULL */
    tlsrec_tls13_secret *binders;         /* may be NULL */
    uint32_t *match;
    tlsrec_key_material *out;             /* staging area of slot `first`, one record per connection; NULL: binder only */
    tlsrec_tls13_secret *early_traffic, *early_exporter;    /* read only with out; early_exporter may be NULL */
    uint32_t count, head, key_cells, psk_len, aligned;
    LadderConsts<T> k;
    LabelW binder, c_e, e_exp;            /* "res binder" or "ext binder", "c e traffic", "e exp master" */
    LadderLabels lb;                      /* key, iv, fin */
};

/* ssl_tls13_offered_psks_check_binder_match (ssl_tls13_server.c:404-457) and,
 * with a.out, ssl_tls13_generate_early_key (ssl_tls13_keys.c:1086-1182), one
 * connection per lane.  Compressions per connection: the binder
 * 14 (Extract 2, midstates 2, binder key 2, midstates 2, finished key 2,
 * midstates 2, MAC 2; the Early Secret's midstates also serve the early
 * secrets); the early keys 10 more (two secrets 4, midstates 2, key 2, iv 2),
 * 8 without the exporter: 14 / 22 / 24.  The two early secrets come before the
 * binder key's midstates so that one pair of midstates is live at a time. */
template <class T> __global__ void __launch_bounds__(64) tls13_early_kernel(Tls13EarlyArgs<T> a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint8_t *conn = reinterpret_cast<const uint8_t *>(a.conns + i);
    const bool cal = (a.aligned & AL_CONNS) != 0;
    W ip[8], op[8], w[16], x[T::HW], tr[T::HW], cs[T::HW];
    {
        /* Early Secret = Extract(0, PSK) */
        uint32_t P[12];
        load_cells<12>(conn, cal, P);
        msg_block<T, 12>(w, P, a.psk_len, 0);
        hmac_block<T>(a.k.zero_ip, a.k.zero_op, w, x);
#pragma unroll
        for (int j = 0; j < 12; j++) P[j] = 0;
    }
    hmac_mid<T>(x, ip, op);
    if (a.out) {
        load_digest<T>(conn + 96, cal, tr);
        label_block<T, OFF_E_TRAFFIC, true>(w, a.c_e, tr);
        hmac_block<T>(ip, op, w, cs);
        store_secret<T>(a.early_traffic + i, (a.aligned & AL_TRAFFIC) != 0, cs);
        if (a.early_exporter) {
            label_block<T, OFF_E_EXP_MASTER, true>(w, a.e_exp, tr);
            hmac_block<T>(ip, op, w, x);
            store_secret<T>(a.early_exporter + i, (a.aligned & AL_AUX) != 0, x);
        }
    }
    /* binder_key = Derive-Secret(Early Secret, "res binder" | "ext binder", ""), then
     * ssl_tls13_calc_finished_core over the truncated ClientHello's hash */
    label_block<T, OFF_BINDER, true>(w, a.binder, a.k.empty);
    hmac_block<T>(ip, op, w, x);
    hmac_mid<T>(x, ip, op);
    label_block<T, OFF_FINISHED, false>(w, a.lb.fin, x);
    hmac_block<T>(ip, op, w, x);
    hmac_mid<T>(x, ip, op);
    load_digest<T>(conn + 48, cal, tr);
    digest_block<T>(w, tr);
    hmac_block<T>(ip, op, w, x);
    if (a.binders) store_secret<T>(a.binders + i, (a.aligned & AL_BINDERS) != 0, x);
    if (a.match) {
        /* mbedtls_ct_memcmp: the OR of the XOR of every cell, no early exit, no branch on the data */
        load_digest<T>(a.offered[i].secret, (a.aligned & AL_OFFERED) != 0, tr);
        W d = 0;
#pragma unroll
        for (int j = 0; j < T::HW; j++) d |= x[j] ^ tr[j];
        uint32_t d32 = (uint32_t) d;
        if constexpr (sizeof(W) == 8) d32 |= (uint32_t) ((uint64_t) d >> 32);
        a.match[i] = d32 == 0 ? 1u : 0u;
    }
    if (a.out) traffic_side<T>(cs, a.lb, a.head, a.key_cells, a.out + i, nullptr, false);
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; tr[j] = 0; cs[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* psk[i] = HKDF-Expand-Label(res_master[i], "resumption", nonce i, H)
 * (ssl_tls13_server.c:3219-3230): 4 compressions.  The 20 bytes of the
 * HkdfLabel up to its context-length byte fill cells 0..4, so the nonce starts
 * on cell 5; its length is wave-uniform, and the 0x01 that closes the
 * HkdfLabel, the 0x80 and the length word (msg_block) move with it. */
struct Tls13TicketArgs {
    const tlsrec_tls13_secret *res_master;
    const uint8_t *nonces;                /* 32 bytes per ticket, nonce_len used */
    tlsrec_tls13_secret *psk;
    uint32_t count, aligned, nonce_len;   /* AL_MASTER res_master, AL_TRANSCRIPT nonces, AL_AUX psk */
    LabelW label;
};

template <class T> __global__ void __launch_bounds__(64) tls13_ticket_kernel(Tls13TicketArgs a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8], w[16], x[T::HW];
    load_digest<T>(a.res_master[i].secret, (a.aligned & AL_MASTER) != 0, x);
    hmac_mid<T>(x, ip, op);
    uint32_t N[8], m[14];
    load_cells<8>(a.nonces + 32 * (size_t) i, (a.aligned & AL_TRANSCRIPT) != 0, N);
#pragma unroll
    for (int c = 0; c < 5; c++) m[c] = a.label.c[c];
#pragma unroll
    for (int c = 0; c < 9; c++) {
        const int rem = (int) a.nonce_len - 4 * c;          /* nonce bytes from this cell on */
        const uint32_t v = c < 8 ? N[c] : 0u;
        uint32_t y;
        if (rem >= 4) y = v;
        else if (rem >= 0) y = (rem ? v & ~(0xffffffffu >> (8 * rem)) : 0u) | (0x01u << (24 - 8 * rem));
        else y = 0u;
        m[5 + c] = y;
    }
    msg_block<T, 14>(w, m, OFF_RESUMPTION + a.nonce_len + 1, 0);
    hmac_block<T>(ip, op, w, x);
    store_secret<T>(a.psk + i, (a.aligned & AL_AUX) != 0, x);
#pragma unroll
    for (int j = 0; j < 8; j++) N[j] = 0;
#pragma unroll
    for (int j = 0; j < 14; j++) m[j] = 0;
#pragma unroll
    for (int j = 0; j < T::HW; j++) x[j] = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* ---- TLS 1.2 / DTLS 1.2 handshake: master secret, Finished verify_data -----
 * ssl_compute_master (ssl_tls.c:6251-6452) and ssl_calc_finished_tls_generic
 * (:7209-7261) with the constant-time check of mbedtls_ssl_parse_finished
 * (:7530), one connection per lane, on the blocks of the ladder above.  Both
 * are PRF(secret, label, seed) = P_hash(secret, label || seed) (RFC 5246
 * section 5) cut to 48 or 12 bytes: two midstates of the secret, then per
 * iteration A(i) = HMAC(A(i-1)) and HMAC(A(i) || label || seed).
 *
 * label || seed, N bytes in the cells S[]:
 *   "master secret" || randbytes              13 + 64 = 77
 *   "extended master secret" || session_hash  22 + 32 = 54, 22 + 48 = 70
 *   "client finished" | "server finished" || transcript hash  15 + 32 = 47, 15 + 48 = 63
 * N is a constant of the instantiation, so the padding and the length word of
 * every block are constants.  Compressions per connection:
 *   A(1): 1, or 2 where N + 9 > 64 (SHA-256, 77);  A(i > 1): 1;  each outer hash: 1
 *   HMAC(A || S): Hash.length + N bytes, 2 inner blocks, or 1 where it pads
 *   into one (SHA-384, 48 + 63 + 17 = 128)
 *   master, SHA-256: 2 + (3 | 2) + 3 + 2 + 3 = 13 | 12, and 2 | 3 more where the
 *   premaster is longer than the block and is hashed first;  SHA-384: 2 + 2 + 3 = 7
 *   verify_data: SHA-256 2 + 2 + 3 = 7;  SHA-384 2 + 2 + 2 = 6 */

/* block `blk` of the n-byte message in m[] (n wave-uniform, blk a constant):
 * bytes past n are masked off.  PAD: the blocks of a plain hash, with 0x80
 * after the message and its length in bits closing the first block that has
 * room for both.  Without PAD the zero-padded block of an HMAC key. */
template <class T, int NC, bool PAD>
__device__ __forceinline__ void key_block(typename T::W (&w)[16], const uint32_t (&m)[NC], uint32_t n, int blk)
{
    constexpr int CPB = T::BB / 4;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int c = 0; c < CPB; c++) {
        const int g = blk * CPB + c;
        const int rem = (int) n - 4 * g;
        const uint32_t v = g < NC ? m[g] : 0u;
        uint32_t x;
        if (rem >= 4) x = v;
        else if (rem > 0) x = (v & ~(0xffffffffu >> (8 * rem))) | (PAD ? 0x80u << (24 - 8 * rem) : 0u);
        else x = PAD && rem == 0 ? 0x80000000u : 0u;
        or_cell<T>(w, c, x);
    }
    const int end = (int) n + 1 + (int) T::LENB;
    if (PAD && end <= (blk + 1) * (int) T::BB && end > blk * (int) T::BB) w[15] = (typename T::W) (n * 8);
}

/* the two midstates of HMAC under the zero-padded key block kb (consumed): 2 compressions */
template <class T>
__device__ __forceinline__ void hmac_mid_block(typename T::W (&kb)[16], typename T::W (&ip)[8], typename T::W (&op)[8])
{
    typedef typename T::W W;
    W w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = kb[j] ^ (W) 0x3636363636363636ULL;
#pragma unroll
    for (int j = 0; j < 8; j++) ip[j] = T::iv(j);
    sha_compress<typename T::S>(ip, w);
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = kb[j] ^ (W) 0x5c5c5c5c5c5c5c5cULL;
#pragma unroll
    for (int j = 0; j < 8; j++) op[j] = T::iv(j);
    sha_compress<typename T::S>(op, w);
#pragma unroll
    for (int j = 0; j < 16; j++) { w[j] = 0; kb[j] = 0; }
}

/* The first OUTC cells of P_hash over the N bytes of S under the midstates ip / op. */
template <class T, int N, int OUTC>
__device__ __forceinline__ void tls12_p_hash(const typename T::W (&ip)[8], const typename T::W (&op)[8],
                                             const uint32_t (&S)[20], uint32_t (&out)[OUTC])
{
    typedef typename T::W W;
    constexpr int ITERS = (4 * OUTC + T::HB - 1) / T::HB;
    constexpr int NC = T::HC + 20, L = T::HB + N;      /* A || S */
    static_assert(N <= 80 && N + 1 + T::LENB <= 2 * T::BB && L + 1 + T::LENB <= 2 * T::BB, "one or two inner blocks");
    W w[16], st[8], A[T::HW];
    uint32_t C[NC];
#pragma unroll
    for (int j = 0; j < T::HC; j++) C[j] = 0;
#pragma unroll
    for (int j = 0; j < 20; j++) C[T::HC + j] = S[j];
#pragma unroll
    for (int j = 0; j < T::HW; j++) A[j] = 0;
#pragma unroll 1
    for (int it = 0; it < ITERS; it++) {
        /* A(it + 1) = HMAC(A(it)); A(0) is S */
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        if (it == 0) {
            msg_block<T, 20>(w, S, N, 0);
            sha_compress<typename T::S>(st, w);
            if constexpr (N + 1 + T::LENB > T::BB) {
                msg_block<T, 20>(w, S, N, 1);
                sha_compress<typename T::S>(st, w);
            }
        } else {
            digest_block<T>(w, A);
            sha_compress<typename T::S>(st, w);
        }
        hmac_outer<T>(op, st, A);
        /* output block = HMAC(A || S) */
#pragma unroll
        for (int c = 0; c < T::HC; c++) C[c] = cell<T, T::HW>(A, c);
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        msg_block<T, NC>(w, C, L, 0);
        sha_compress<typename T::S>(st, w);
        if constexpr (L + 1 + T::LENB > T::BB) {
            msg_block<T, NC>(w, C, L, 1);
            sha_compress<typename T::S>(st, w);
        }
        W D[T::HW];
        hmac_outer<T>(op, st, D);
#pragma unroll
        for (int q = 0; q < ITERS; q++) {
            if (it == q) {
#pragma unroll
                for (int c = 0; c < T::HC; c++)
                    if (q * T::HC + c < OUTC) out[q * T::HC + c] = cell<T, T::HW>(D, c);
            }
        }
#pragma unroll
        for (int j = 0; j < T::HW; j++) D[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = 0;
#pragma unroll
    for (int j = 0; j < T::HW; j++) A[j] = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int j = 0; j < NC; j++) C[j] = 0;
}

struct Tls12MasterArgs {
    const tlsrec_tls12_pms_conn *conns;
    tlsrec_tls12_conn *out;
    uint32_t count, pms_len, aligned;     /* AL_CONNS conns, AL_AUX out */
};

/* EMS: "extended master secret" over the session hash (RFC 7627 section 4,
 * ssl_tls.c:6284-6305), else "master secret" over randbytes (:6269).  The
 * premaster is the HMAC key: zero-padded to the block, or under SHA-256 its
 * digest where it is longer than 64 bytes (RFC 2104; two inner blocks up to
 * 119 bytes, three from 120).  Only the 16-byte groups that hold premaster
 * bytes are loaded. */
template <class T, bool EMS> __global__ void __launch_bounds__(64) tls12_master_kernel(Tls12MasterArgs a)
{
    typedef typename T::W W;
    static_assert(sizeof(tlsrec_tls12_pms_conn) == 240 && offsetof(tlsrec_tls12_pms_conn, randbytes) == 128 &&
                  offsetof(tlsrec_tls12_pms_conn, session_hash) == 192 && sizeof(tlsrec_tls12_conn) == 112,
                  "tlsrec_tls12_pms_conn / tlsrec_tls12_conn layout");
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint8_t *conn = reinterpret_cast<const uint8_t *>(a.conns + i);
    const bool cal = (a.aligned & AL_CONNS) != 0;
    const uint32_t n = a.pms_len;
    W ip[8], op[8], w[16];
    /* every load of the connection is issued before the first compression: one wait on memory, not three */
    uint32_t R[16], S[20], X[12], Hs[EMS ? (int) T::HC : 1];
    load_cells<16>(conn + 128, cal, R);
    if constexpr (EMS) load_cells<T::HC>(conn + 192, cal, Hs);
    {
        uint32_t P[32];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uint32_t g[4] = { 0u, 0u, 0u, 0u };
            if ((uint32_t) (16 * k) < n) load_cells<4>(conn + 16 * k, cal, g);
#pragma unroll
            for (int j = 0; j < 4; j++) { P[4 * k + j] = g[j]; g[j] = 0; }
        }
        W kb[16];
        bool hashed = false;
        if constexpr (sizeof(W) == 4) hashed = n > T::BB;
        if (hashed) {
            W st[8];
#pragma unroll
            for (int j = 0; j < 8; j++) st[j] = T::iv(j);
            key_block<T, 32, true>(w, P, n, 0);
            sha_compress<typename T::S>(st, w);
            key_block<T, 32, true>(w, P, n, 1);
            sha_compress<typename T::S>(st, w);
            if (n + 1 + T::LENB > 2 * T::BB) {
                key_block<T, 32, true>(w, P, n, 2);
                sha_compress<typename T::S>(st, w);
            }
#pragma unroll
            for (int j = 0; j < 16; j++) kb[j] = j < T::HW ? st[j] : (W) 0;
#pragma unroll
            for (int j = 0; j < 8; j++) st[j] = 0;
        } else {
            key_block<T, 32, false>(kb, P, n, 0);
        }
#pragma unroll
        for (int j = 0; j < 32; j++) P[j] = 0;
        hmac_mid_block<T>(kb, ip, op);
    }
    constexpr int N = EMS ? 22 + (int) T::HB : 77;
    if constexpr (EMS) {
        S[0] = 0x65787465u;      /* "exte" */
        S[1] = 0x6e646564u;      /* "nded" */
        S[2] = 0x206d6173u;      /* " mas" */
        S[3] = 0x74657220u;      /* "ter " */
        S[4] = 0x73656372u;      /* "secr" */
        S[5] = 0x65740000u | (Hs[0] >> 16);     /* "et" */
#pragma unroll
        for (int k = 1; k < T::HC; k++) S[5 + k] = (Hs[k - 1] << 16) | (Hs[k] >> 16);
        S[5 + T::HC] = Hs[T::HC - 1] << 16;
#pragma unroll
        for (int k = 6 + T::HC; k < 20; k++) S[k] = 0;
    } else {
        S[0] = 0x6d617374u;      /* "mast" */
        S[1] = 0x65722073u;      /* "er s" */
        S[2] = 0x65637265u;      /* "ecre" */
        S[3] = 0x74000000u | (R[0] >> 8);       /* "t" */
#pragma unroll
        for (int k = 1; k < 16; k++) S[3 + k] = (R[k - 1] << 24) | (R[k] >> 8);
        S[19] = R[15] << 24;
    }
    tls12_p_hash<T, N, 12>(ip, op, S, X);
    /* master || server_random || client_random: the swap of ssl_tls.c:6479-6488 */
    uint32_t o[28];
#pragma unroll
    for (int c = 0; c < 12; c++) o[c] = __builtin_bswap32(X[c]);
#pragma unroll
    for (int c = 0; c < 8; c++) { o[12 + c] = __builtin_bswap32(R[8 + c]); o[20 + c] = __builtin_bswap32(R[c]); }
    if (a.aligned & AL_AUX) {
        uint4 *q = reinterpret_cast<uint4 *>(a.out + i);
#pragma unroll
        for (int k = 0; k < 7; k++) q[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else {
        uint8_t *b = reinterpret_cast<uint8_t *>(a.out + i);
#pragma unroll
        for (int c = 0; c < 28; c++) {
            b[4 * c] = (uint8_t) o[c]; b[4 * c + 1] = (uint8_t) (o[c] >> 8);
            b[4 * c + 2] = (uint8_t) (o[c] >> 16); b[4 * c + 3] = (uint8_t) (o[c] >> 24);
        }
    }
#pragma unroll
    for (int j = 0; j < 12; j++) { X[j] = 0; o[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int j = 0; j < 20; j++) S[j] = 0;
}

enum { AL_VERIFY = AL_AUX, AL_OFFERED12 = AL_TRAFFIC };

struct Tls12FinishedArgs {
    const tlsrec_tls12_conn *conns;       /* master only */
    const tlsrec_tls13_secret *transcripts;
    const uint8_t *offered;               /* 16 bytes per connection, 12 compared; with match, or both NULL */
    uint8_t *verify;                      /* 16 bytes per connection; may be NULL */
    uint32_t *match;
    uint32_t count, aligned, l0, l1;      /* l0, l1: "clie" "nt f" or "serv" "er f" */
};

template <class T> __global__ void __launch_bounds__(64) tls12_finished_kernel(Tls12FinishedArgs a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8];
    /* every load is issued before the first compression */
    uint32_t Hs[T::HC], S[20], X[3], O[3] = { 0u, 0u, 0u };
    load_cells<T::HC>(a.transcripts[i].secret, (a.aligned & AL_TRANSCRIPT) != 0, Hs);
    if (a.match) load_cells<3>(a.offered + 16 * (size_t) i, (a.aligned & AL_OFFERED12) != 0, O);
    {
        uint32_t M[12];
        W kb[16];
        load_cells<12>(reinterpret_cast<const uint8_t *>(a.conns + i), (a.aligned & AL_CONNS) != 0, M);
        key_block<T, 12, false>(kb, M, 48, 0);
#pragma unroll
        for (int j = 0; j < 12; j++) M[j] = 0;
        hmac_mid_block<T>(kb, ip, op);
    }
    S[0] = a.l0;
    S[1] = a.l1;
    S[2] = 0x696e6973u;          /* "inis" */
    S[3] = 0x68656400u | (Hs[0] >> 24);         /* "hed" */
#pragma unroll
    for (int k = 1; k < T::HC; k++) S[3 + k] = (Hs[k - 1] << 8) | (Hs[k] >> 24);
    S[3 + T::HC] = Hs[T::HC - 1] << 8;
#pragma unroll
    for (int k = 4 + T::HC; k < 20; k++) S[k] = 0;
    tls12_p_hash<T, 15 + (int) T::HB, 3>(ip, op, S, X);
    if (a.verify) {
        uint8_t *b = a.verify + 16 * (size_t) i;
        if (a.aligned & AL_VERIFY) {
            *reinterpret_cast<uint4 *>(b) = make_uint4(__builtin_bswap32(X[0]), __builtin_bswap32(X[1]),
                                                       __builtin_bswap32(X[2]), 0u);
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t v = c < 3 ? X[c] : 0u;
                b[4 * c] = (uint8_t) (v >> 24); b[4 * c + 1] = (uint8_t) (v >> 16);
                b[4 * c + 2] = (uint8_t) (v >> 8); b[4 * c + 3] = (uint8_t) v;
            }
        }
    }
    if (a.match) {
        /* mbedtls_ct_memcmp over 12 bytes: the OR of the XOR of the three cells, no early exit, no branch on the data */
        const uint32_t d = (X[0] ^ O[0]) | (X[1] ^ O[1]) | (X[2] ^ O[2]);
        a.match[i] = d == 0 ? 1u : 0u;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) X[j] = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 20; j++) S[j] = 0;
}

/* ---- keying material exporters (RFC 8446 7.5, RFC 5705) ---------------------
 * mbedtls_ssl_tls13_exporter (ssl_tls13_keys.c:1828-1858) and
 * mbedtls_ssl_tls12_export_keying_material (ssl_tls.c:8886-8936), one connection
 * per lane, on the blocks above.  Unlike the rest of the family the shapes are
 * not fixed: the label (up to 249 bytes), the context (up to 255) and the output
 * (up to 8160) are run-time values, the same for every lane of a call, so the
 * loops over their blocks are rolled and their trip counts are scalar.
 *
 * What is the same for every connection is built on the host: in TLS 1.3 the
 * whole padded inner message of the first Expand-Label (exporter_blocks(), a
 * kernel argument) and the "exporter" HkdfLabel prefix.  What is per connection
 * and public -- the context, the randoms, the assembled PRF seed -- is staged in
 * LDS as big-endian cells, cell g of lane l at pub[g * 64 + l]: a wave's access
 * to one cell falls in 64 different banks, a rolled loop can index it, and a
 * lane touches its own column only, so there is no barrier.  What is secret
 * (the exporter secret, the master secret, every midstate, S1, A(i), T(k)) is in
 * registers only; each output block is stored as soon as it is made.
 *
 * Compressions per connection (exporters), with b(n) = ceil((n + 1 + LENB) / BB),
 * iters = ceil(out_len / H), L the label's length, C the context's:
 *   TLS 1.3: 2 + (b(11 + L + H) + 1) + 2 + (C ? b(C) : 0) + 2 + 3 (iters - 1)
 *   TLS 1.2, N = L + 64 (+ 2 + C): 2 + (b(N) + 1) + iters (b(H + N) + 1) + 2 (iters - 1) */
enum { EXP13_CELLS = 64, EXP12_CELLS = 160 };

/* byte p of the lane's column */
__device__ __forceinline__ void pub_put(uint32_t *pub, uint32_t p, uint32_t byte)
{
    reinterpret_cast<uint8_t *>(pub + (p >> 2) * 64 + threadIdx.x)[3 - (p & 3)] = (uint8_t) byte;
}

/* 0x80 after a message of n bytes, and zeros to the end of its cell */
__device__ __forceinline__ void pub_close(uint32_t *pub, uint32_t n)
{
    pub_put(pub, n, 0x80);
    for (uint32_t p = n + 1; p & 3; p++) pub_put(pub, p, 0);
}

/* One block of a padded message out of the lane's column: cells FROM.. of the
 * block that starts at cell `first`; cells from `lim` on are zero, and `bits`
 * closes the block when it is the last.  Cells below FROM are left zero for the
 * caller.  first, lim and last are wave-uniform. */
template <class T, int FROM, int CELLS>
__device__ __forceinline__ void pub_block(typename T::W (&w)[16], const uint32_t *pub, uint32_t first, uint32_t lim,
                                          bool last, uint32_t bits)
{
    constexpr int CPB = T::BB / 4;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int c = FROM; c < CPB; c++) {
        const uint32_t g = first + c;
        const uint32_t v = pub[(g < CELLS ? g : CELLS - 1) * 64 + threadIdx.x];
        or_cell<T>(w, c, g < lim ? v : 0u);
    }
    if (last) w[15] = (typename T::W) bits;
}

/* `take` (1..H, wave-uniform) bytes of x to dst: 16-byte stores for the whole groups if al16, bytes otherwise */
template <class T>
__device__ __forceinline__ void store_out(uint8_t *dst, bool al16, const typename T::W (&x)[T::HW], uint32_t take)
{
#pragma unroll
    for (int g = 0; g < T::HB / 16; g++) {
        uint32_t m[4];
#pragma unroll
        for (int j = 0; j < 4; j++) m[j] = __builtin_bswap32(cell<T, T::HW>(x, 4 * g + j));
        if (al16 && take >= 16u * g + 16u) {
            *reinterpret_cast<uint4 *>(dst + 16 * g) = make_uint4(m[0], m[1], m[2], m[3]);
        } else {
#pragma unroll
            for (int b = 0; b < 16; b++)
                if (16u * g + b < take) dst[16 * g + b] = (uint8_t) (m[b >> 2] >> (8 * (b & 3)));
        }
#pragma unroll
        for (int j = 0; j < 4; j++) m[j] = 0;
    }
}

enum { OFF_EXPORTER = 18, AL_OUT = AL_AUX, AL_SECRETS = AL_MASTER };

template <class T> struct Tls13ExporterArgs {
    const tlsrec_tls13_secret *secrets;
    const uint8_t *contexts;
    uint8_t *out;
    uint32_t count, context_len, context_stride, out_len, out_stride, aligned, nblk;
    LabelW label;                          /* HkdfLabel(out_len, "exporter", a context of H bytes) */
    typename T::W empty[T::HW];            /* Hash("") */
    typename T::W words[T::BB == 64 ? 80 : 48];   /* HkdfLabel(H, label, Hash("")) || 0x01, padded: nblk blocks */
};

template <class T> __global__ void __launch_bounds__(64) tls13_exporter_kernel(Tls13ExporterArgs<T> a)
{
    typedef typename T::W W;
    constexpr int CPB = T::BB / 4;
    constexpr int EC = 5 + T::HC, NC = T::HC + EC, LK = 2 * T::HB + OFF_EXPORTER + 1;
    static_assert(LK + 1 + T::LENB > T::BB && LK + 1 + T::LENB <= 2 * T::BB, "T(k > 1) takes two inner blocks");
    __shared__ uint32_t pub[EXP13_CELLS * 64];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8], w[16], st[8], x[T::HW], hc[T::HW];
    load_digest<T>(a.secrets[i].secret, (a.aligned & AL_SECRETS) != 0, x);
    const uint32_t n = a.context_len;
    if (n) {
        const uint8_t *c = a.contexts + (size_t) i * a.context_stride;
#pragma unroll 1
        for (uint32_t p = 0; p < n; p++) pub_put(pub, p, c[p]);
        pub_close(pub, n);
    }
    /* S1 = Expand-Label(secret, label, Hash(""), H): the same inner message for every lane */
    hmac_mid<T>(x, ip, op);
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = ip[j];
#pragma unroll 1
    for (uint32_t b = 0; b < a.nblk; b++) {
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = a.words[16 * b + j];
        sha_compress<typename T::S>(st, w);
    }
    hmac_outer<T>(op, st, x);
    hmac_mid<T>(x, ip, op);
    /* Hash(context) */
    if (n) {
        const uint32_t nb = (n + 1 + T::LENB + T::BB - 1) / T::BB, lim = (n + 4) / 4;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = T::iv(j);
#pragma unroll 1
        for (uint32_t b = 0; b < nb; b++) {
            pub_block<T, 0, EXP13_CELLS>(w, pub, b * CPB, lim, b + 1 == nb, n * 8);
            sha_compress<typename T::S>(st, w);
        }
#pragma unroll
        for (int j = 0; j < T::HW; j++) hc[j] = st[j];
    } else {
#pragma unroll
        for (int j = 0; j < T::HW; j++) hc[j] = a.empty[j];
    }
    /* T(1) = HMAC(S1, HkdfLabel || 0x01): one inner block */
    uint8_t *dst = a.out + (size_t) i * a.out_stride;
    const bool oal = (a.aligned & AL_OUT) != 0;
    uint32_t left = a.out_len;
    label_block<T, OFF_EXPORTER, true>(w, a.label, hc);
    hmac_block<T>(ip, op, w, x);
    store_out<T>(dst, oal, x, left < T::HB ? left : (uint32_t) T::HB);
    /* T(k) = HMAC(S1, T(k - 1) || HkdfLabel || k): H + 18 + H + 1 bytes, two inner blocks */
    uint32_t E[EC];
#pragma unroll
    for (int c = 0; c < 4; c++) E[c] = a.label.c[c];
    E[4] = a.label.c[4] | (cell<T, T::HW>(hc, 0) >> 16);
#pragma unroll
    for (int k = 1; k < T::HC; k++) E[4 + k] = (cell<T, T::HW>(hc, k - 1) << 16) | (cell<T, T::HW>(hc, k) >> 16);
    E[4 + T::HC] = cell<T, T::HW>(hc, T::HC - 1) << 16;
#pragma unroll 1
    for (uint32_t k = 2; left > T::HB; k++) {
        left -= T::HB;
        dst += T::HB;
        uint32_t M[NC];
#pragma unroll
        for (int c = 0; c < T::HC; c++) M[c] = cell<T, T::HW>(x, c);
#pragma unroll
        for (int c = 0; c < EC; c++) M[T::HC + c] = E[c];
        M[NC - 1] |= k << 8;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        msg_block<T, NC>(w, M, LK, 0);
        sha_compress<typename T::S>(st, w);
        msg_block<T, NC>(w, M, LK, 1);
        sha_compress<typename T::S>(st, w);
        hmac_outer<T>(op, st, x);
        store_out<T>(dst, oal, x, left < T::HB ? left : (uint32_t) T::HB);
#pragma unroll
        for (int c = 0; c < T::HC; c++) M[c] = 0;
    }
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; hc[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; st[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

struct Tls12ExportArgs {
    const tlsrec_tls12_conn *conns;
    const uint8_t *contexts;
    uint8_t *out;
    uint32_t count, label_len, context_len, context_stride, use_context, out_len, out_stride, aligned;
    uint32_t label[63];                   /* big-endian cells, zero-padded */
};

/* P_hash(master, S) with S = label || client_random || server_random
 * [|| uint16(context_len) || context], N bytes, staged from cell HC of the lane's
 * column on: the inner message of A(1) is S, that of an output block is A(i) || S,
 * whose first HC cells come from registers and whose rest is the same column read
 * from cell HC on. */
template <class T> __global__ void __launch_bounds__(64) tls12_export_kernel(Tls12ExportArgs a)
{
    typedef typename T::W W;
    constexpr int CPB = T::BB / 4;
    constexpr uint32_t S0 = 4 * T::HC;    /* the byte of the column at which S starts */
    __shared__ uint32_t pub[EXP12_CELLS * 64];
    static_assert(T::HC + (249 + 64 + 2 + 255 + 4) / 4 <= EXP12_CELLS, "the longest seed fits the column");
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint8_t *conn = reinterpret_cast<const uint8_t *>(a.conns + i);
    const bool cal = (a.aligned & AL_CONNS) != 0;
    W ip[8], op[8], w[16], st[8], A[T::HW], D[T::HW];
    uint32_t R[16];
    load_cells<16>(conn + 48, cal, R);
    {
        uint32_t M[12];
        W kb[16];
        load_cells<12>(conn, cal, M);
        key_block<T, 12, false>(kb, M, 48, 0);
#pragma unroll
        for (int j = 0; j < 12; j++) M[j] = 0;
        hmac_mid_block<T>(kb, ip, op);
    }
    /* the seed: the label by cells, then bytes */
#pragma unroll 1
    for (uint32_t c = 0; 4 * c < a.label_len; c++) pub[(T::HC + c) * 64 + threadIdx.x] = a.label[c];
    uint32_t p = S0 + a.label_len;
    /* randbytes is server_random || client_random: client_random goes first (ssl_tls.c:8920-8925) */
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t v = R[(k + 8) & 15];
#pragma unroll
        for (int j = 0; j < 4; j++) pub_put(pub, p + 4 * k + j, v >> (24 - 8 * j));
    }
    p += 64;
    if (a.use_context) {
        pub_put(pub, p, a.context_len >> 8);
        pub_put(pub, p + 1, a.context_len);
        p += 2;
        const uint8_t *c = a.contexts + (size_t) i * a.context_stride;
#pragma unroll 1
        for (uint32_t q = 0; q < a.context_len; q++) pub_put(pub, p + q, c[q]);
        p += a.context_len;
    }
    pub_close(pub, p);
    const uint32_t N = p - S0, lim = (p + 4) / 4;
    /* A(1) = HMAC(master, S) */
    {
        const uint32_t nb = (N + 1 + T::LENB + T::BB - 1) / T::BB;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
#pragma unroll 1
        for (uint32_t b = 0; b < nb; b++) {
            pub_block<T, 0, EXP12_CELLS>(w, pub, T::HC + b * CPB, lim, b + 1 == nb, (T::BB + N) * 8);
            sha_compress<typename T::S>(st, w);
        }
        hmac_outer<T>(op, st, A);
    }
    uint8_t *dst = a.out + (size_t) i * a.out_stride;
    const bool oal = (a.aligned & AL_OUT) != 0;
    const uint32_t nb = (T::HB + N + 1 + T::LENB + T::BB - 1) / T::BB, bits = (T::BB + T::HB + N) * 8;
    uint32_t left = a.out_len;
#pragma unroll 1
    for (;;) {
        /* output block = HMAC(master, A(i) || S) */
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        pub_block<T, T::HC, EXP12_CELLS>(w, pub, 0, lim, nb == 1, bits);
#pragma unroll
        for (int c = 0; c < T::HC; c++) or_cell<T>(w, c, cell<T, T::HW>(A, c));
        sha_compress<typename T::S>(st, w);
#pragma unroll 1
        for (uint32_t b = 1; b < nb; b++) {
            pub_block<T, 0, EXP12_CELLS>(w, pub, b * CPB, lim, b + 1 == nb, bits);
            sha_compress<typename T::S>(st, w);
        }
        hmac_outer<T>(op, st, D);
        store_out<T>(dst, oal, D, left < T::HB ? left : (uint32_t) T::HB);
        if (left <= T::HB) break;
        left -= T::HB;
        dst += T::HB;
        /* A(i + 1) = HMAC(master, A(i)) */
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        digest_block<T>(w, A);
        sha_compress<typename T::S>(st, w);
        hmac_outer<T>(op, st, A);
    }
#pragma unroll
    for (int j = 0; j < T::HW; j++) { A[j] = 0; D[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; st[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* ======================================================================
 * DTLS cookies (library/ssl_cookie.c, ssl_msg.c:3322-3454)
 * ====================================================================== */
/* mbedtls_ssl_cookie_write / _check and mbedtls_ssl_check_dtls_clihlo_cookie,
 * one client per lane, all under the one key whose two HMAC midstates the
 * context holds (uniform loads: scalar registers, read once per wave).
 *     cookie = BE32(t) || HMAC-SHA256(key, BE32(t) || id)[0..28)
 * The inner message is 4 + id_len bytes: one block up to an id of 51 bytes
 * (an IPv4 or IPv6 address with its port), built with constant word indices;
 * a longer id takes further blocks in a loop whose trip count differs between
 * the lanes of a wave.  Compressions per item: write and check 2 (+1 per
 * further block), a ClientHello 2 when its cookie passes or cannot be one
 * (length != 32), 4 when a 32-byte cookie fails.  The kernel has one MAC site:
 * in a wave of ClientHellos the lanes that check and the lanes that only
 * write run it together, and only a failed 32-byte cookie costs a second trip. */
enum { CK_WRITE = 0, CK_CHECK = 1, CK_HELLO = 2 };

struct CookieArgs {
    const uint32_t *mid;          /* ip[8], op[8] */
    const void *items;            /* tlsrec_cookie_item / tlsrec_clihlo */
    const uint8_t *arena;         /* check: the cookies; hello: the datagrams */
    const uint8_t *id_arena;
    uint8_t *out;                 /* write: the cookies; hello: the HelloVerifyRequests */
    int32_t *status;              /* int32 per item; hello: tlsrec_clihlo_res */
    uint64_t now;
    uint32_t timeout, n;
};

/* fail closed: what the kernel does not reach reads INTERNAL_ERROR (words = int32s per result) */
__global__ void __launch_bounds__(64) cookie_prefill_kernel(int32_t *status, uint32_t n, uint32_t words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    status[(size_t) i * words] = TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (words == 2) status[(size_t) i * 2 + 1] = 0;
}

/* the key's midstates, once per context; the staged key is zeroed behind them */
__global__ void __launch_bounds__(64) cookie_setup_kernel(uint32_t *mid, uint8_t *key)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t k[8], ip[8], op[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = load_be32(key + 4 * j, false);
    hmac_mid<L256>(k, ip, op);
#pragma unroll
    for (int j = 0; j < 8; j++) { mid[j] = ip[j]; mid[8 + j] = op[j]; }
    for (int j = 0; j < 32; j++) key[j] = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { k[j] = 0; ip[j] = 0; op[j] = 0; }
}

/* big-endian word of the padded id at byte p: id bytes below id_len (no byte
 * at or past it is read), 0x80 at id_len, zero after */
__device__ __forceinline__ uint32_t cookie_id_word(const uint8_t *id, int p, int id_len)
{
    const int rem = id_len - p;
    uint32_t v = 0;
    if (rem >= 4) {
        v = load_be32(id + p, false);
    } else if (rem >= 0) {
        if (rem > 0) v |= (uint32_t) id[p] << 24;
        if (rem > 1) v |= (uint32_t) id[p + 1] << 16;
        if (rem > 2) v |= (uint32_t) id[p + 2] << 8;
        v |= 0x80u << (24 - 8 * rem);
    }
    return v;
}

/* HMAC-SHA256(key, BE32(t) || id) from the midstates; mac[0..7) is the cookie's MAC */
__device__ __forceinline__ void cookie_mac(const uint32_t (&ip)[8], const uint32_t (&op)[8], uint32_t t,
                                           const uint8_t *id, uint32_t id_len, uint32_t (&mac)[8])
{
    uint32_t st[8], w[16];
    const uint32_t n = 4 + id_len, nblk = (n + 9 + 63) >> 6;
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = ip[j];
    w[0] = t;
#pragma unroll
    for (int c = 1; c < 16; c++) w[c] = cookie_id_word(id, 4 * c - 4, (int) id_len);
    if (nblk == 1) w[15] = (64 + n) * 8;
    sha_compress<S256>(st, w);
#pragma unroll 1
    for (uint32_t b = 1; b < nblk; b++) {
#pragma unroll
        for (int c = 0; c < 16; c++) w[c] = cookie_id_word(id, (int) (64 * b) + 4 * c - 4, (int) id_len);
        if (b == nblk - 1) w[15] = (64 + n) * 8;
        sha_compress<S256>(st, w);
    }
    hmac_outer<L256>(op, st, mac);
}

/* N big-endian words to any address: 4-byte stores, or bytes */
template <int N> __device__ __forceinline__ void cookie_store(uint8_t *p, const uint32_t (&v)[N])
{
    if (((uintptr_t) p & 3) == 0) {
#pragma unroll
        for (int c = 0; c < N; c++) reinterpret_cast<uint32_t *>(p)[c] = __builtin_bswap32(v[c]);
    } else {
#pragma unroll
        for (int c = 0; c < N; c++) {
            p[4 * c] = (uint8_t) (v[c] >> 24); p[4 * c + 1] = (uint8_t) (v[c] >> 16);
            p[4 * c + 2] = (uint8_t) (v[c] >> 8); p[4 * c + 3] = (uint8_t) v[c];
        }
    }
}

/* a ClientHello whose cookie did not pass: the buffer checks of ssl_msg.c:3424 and of f_cookie_write
 * (:3436-3440; it also refuses an id it cannot take); write = a HelloVerifyRequest follows */
__device__ __forceinline__ void cookie_hvr_room(uint32_t out_cap, uint32_t id_len, int32_t &st, bool &write)
{
    st = out_cap < 28 ? TLSREC_ERR_SSL_BUFFER_TOO_SMALL : TLSREC_ERR_SSL_INTERNAL_ERROR;
    write = out_cap >= TLSREC_DTLS_HVR_LEN && id_len <= 255;
}

template <int MODE> __global__ void __launch_bounds__(64) cookie_kernel(CookieArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    uint32_t ip[8], op[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = a.mid[j]; op[j] = a.mid[8 + j]; }
    const uint32_t now32 = (uint32_t) a.now;                     /* MBEDTLS_PUT_UINT32_BE(t), ssl_cookie.c:140 */

    const uint8_t *id, *in = nullptr;
    uint8_t *out = nullptr;
    uint32_t id_len, out_cap = 0;
    uint32_t C[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };          /* the received cookie */
    int32_t st = 0;
    bool check = false, write = false;
    if constexpr (MODE == CK_HELLO) {
        const tlsrec_clihlo h = static_cast<const tlsrec_clihlo *>(a.items)[i];
        in = a.arena + h.off;
        id = a.id_arena + h.id_off;
        id_len = h.id_len;
        out = a.out + h.out_off;
        out_cap = h.out_cap;
        const uint32_t len = h.len;
        /* ssl_msg.c:3360-3393; every byte read lies below len */
        bool bad = len < 61;
        uint32_t ck_at = 0, ck_len = 0;
        if (!bad) {
            const uint32_t epoch = ((uint32_t) in[3] << 8) | in[4];
            const uint32_t frag = ((uint32_t) in[19] << 16) | ((uint32_t) in[20] << 8) | in[21];
            const uint32_t sid_len = in[59];
            bad = in[0] != 22 || epoch != 0 || frag != 0 || 61 + sid_len > len;
            if (!bad) {
                ck_len = in[60 + sid_len];
                ck_at = 61 + sid_len;
                bad = ck_at + ck_len > len;
            }
        }
        if (bad) {
            st = TLSREC_ERR_SSL_DECODE_ERROR;
        } else if (ck_len == TLSREC_COOKIE_LEN && id_len <= 255) {
            const uint8_t *ck = in + ck_at;
            const bool al4 = ((uintptr_t) ck & 3) == 0;
#pragma unroll
            for (int c = 0; c < 8; c++) C[c] = load_be32(ck + 4 * c, al4);
            check = true;
        } else {
            write = true;        /* f_cookie_check != 0: the HelloVerifyRequest path */
        }
    } else {
        const tlsrec_cookie_item it = static_cast<const tlsrec_cookie_item *>(a.items)[i];
        id = a.id_arena + it.id_off;
        id_len = it.id_len;
        if (id_len > 255) {
            st = TLSREC_ERR_SSL_BAD_INPUT_DATA;
        } else if (MODE == CK_WRITE) {
            out = a.out + it.cookie_off;
            if (it.cookie_len < TLSREC_COOKIE_LEN) st = TLSREC_ERR_SSL_BUFFER_TOO_SMALL;     /* ssl_cookie.c:132 */
            else write = true;
        } else if (it.cookie_len != TLSREC_COOKIE_LEN) {
            st = -1;                                                                         /* ssl_cookie.c:198-200 */
        } else {
            const uint8_t *ck = a.arena + it.cookie_off;
            const bool al4 = ((uintptr_t) ck & 3) == 0;
#pragma unroll
            for (int c = 0; c < 8; c++) C[c] = load_be32(ck + 4 * c, al4);
            check = true;
        }
    }

    /* One MAC site, at most two passes.  Pass 0: the lanes with a cookie to check hash under its time
     * stamp, the lanes that only write (no cookie of 32 bytes came) under `now`, side by side.  Pass 1
     * (ClientHellos only): the lanes whose cookie failed hash again under `now` for the new cookie. */
    uint32_t olen = 0;
    uint32_t mac[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    if (MODE == CK_HELLO && write) cookie_hvr_room(out_cap, id_len, st, write);
#pragma unroll 1
    for (int pass = 0; pass < (MODE == CK_HELLO ? 2 : 1); pass++) {
        const bool chk = MODE != CK_WRITE && pass == 0 && check;
        if (!chk && !(MODE != CK_CHECK && write)) continue;
        cookie_mac(ip, op, chk ? C[0] : now32, id, id_len, mac);
        if (chk) {
            /* mbedtls_ct_memcmp over 28 bytes: the OR of the XOR of the seven words, no early exit; the
             * statuses are selected, not branched on (ssl_cookie.c:222-242) */
            uint32_t d = 0;
#pragma unroll
            for (int c = 0; c < 7; c++) d |= mac[c] ^ C[1 + c];
            const uint64_t age = a.now - (uint64_t) C[0];
            const int32_t late = (a.timeout != 0 && age > (uint64_t) a.timeout) ? -1 : 0;
            st = d != 0 ? TLSREC_ERR_SSL_INVALID_MAC : late;
            if (MODE == CK_HELLO && st != 0) cookie_hvr_room(out_cap, id_len, st, write);
        } else if (MODE == CK_WRITE) {
            const uint32_t o[8] = { now32, mac[0], mac[1], mac[2], mac[3], mac[4], mac[5], mac[6] };
            cookie_store<8>(out, o);
            write = false;
        } else {
            /* ssl_msg.c:3429-3451 with olen = 60: bytes 0-10 and 17-21 of the input, length 47, type 3,
             * length and fragment_length 35, FE FF, cookie length 32, the cookie */
            uint32_t b[25];
#pragma unroll
            for (int k = 0; k < 25; k++) b[k] = (k < 11 || (k >= 17 && k < 22)) ? in[k] : 0u;
            const uint32_t o[15] = {
                (b[0] << 24) | (b[1] << 16) | (b[2] << 8) | b[3],
                (b[4] << 24) | (b[5] << 16) | (b[6] << 8) | b[7],
                (b[8] << 24) | (b[9] << 16) | (b[10] << 8),
                ((TLSREC_DTLS_HVR_LEN - 13u) << 24) | (3u << 16),
                ((TLSREC_DTLS_HVR_LEN - 25u) << 24) | (b[17] << 16) | (b[18] << 8) | b[19],
                (b[20] << 24) | (b[21] << 16),
                ((TLSREC_DTLS_HVR_LEN - 25u) << 24) | 0x00feff00u | TLSREC_COOKIE_LEN,
                now32, mac[0], mac[1], mac[2], mac[3], mac[4], mac[5], mac[6] };
            cookie_store<15>(out, o);
            st = TLSREC_ERR_SSL_HELLO_VERIFY_REQUIRED;
            olen = TLSREC_DTLS_HVR_LEN;
            write = false;
        }
    }
    if (MODE == CK_HELLO) {
        a.status[2 * (size_t) i] = st;
        a.status[2 * (size_t) i + 1] = (int32_t) olen;
    } else {
        a.status[i] = st;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; mac[j] = 0; }
}

} /* namespace tlsks */

using namespace tlsks;

/* ======================================================================
 * host side
 * ==================================================================== */
static const size_t MAX_LABEL = 249;        /* MBEDTLS_SSL_TLS1_3_HKDF_LABEL_MAX_LABEL_LEN, ssl_tls13_keys.h:66 */
static const size_t MAX_CONTEXT = 64;       /* MBEDTLS_SSL_TLS1_3_KEY_SCHEDULE_MAX_CONTEXT_LEN = PSA_HASH_MAX_SIZE */
static const size_t MAX_EXPANSION = 255 * 64;   /* ..._MAX_EXPANSION_LEN = 255 * MBEDTLS_TLS1_3_MD_MAX_SIZE */

static int alg_index(int hash_alg)
{
    return hash_alg == TLSREC_ALG_SHA_256 ? H_SHA256 : hash_alg == TLSREC_ALG_SHA_384 ? H_SHA384 : -1;
}

static size_t alg_len(int idx) { return idx == H_SHA384 ? 48 : 32; }

/* ssl_tls13_hkdf_encode_label, ssl_tls13_keys.c:98-136 (without the context
 * bytes when ctx == NULL: the caller appends a device-computed context) */
static size_t encode_label(size_t desired, const unsigned char *label, size_t label_len, const unsigned char *ctx,
                           size_t ctx_len, uint8_t *dst)
{
    uint8_t *p = dst;
    *p++ = (uint8_t) (desired >> 8);
    *p++ = (uint8_t) desired;
    *p++ = (uint8_t) (6 + label_len);
    memcpy(p, "tls13 ", 6);
    p += 6;
    if (label_len) memcpy(p, label, label_len);
    p += label_len;
    *p++ = (uint8_t) ctx_len;
    if (ctx && ctx_len) {
        memcpy(p, ctx, ctx_len);
        p += ctx_len;
    }
    return (size_t) (p - dst);
}

/* A device arena for single-shot calls: inputs are packed into one host
 * buffer, copied once, the job chain runs, the outputs come back. */
namespace {
struct Arena {
    uint8_t host[32768];
    size_t used = 0;
    size_t put(const void *p, size_t n)
    {
        size_t off = used;
        if (n && p) memcpy(host + off, p, n);
        else if (n) memset(host + off, 0, n);
        used = (used + n + 15) & ~(size_t) 15;
        return off;
    }
};
}

static pthread_mutex_t g_ks_mu = PTHREAD_MUTEX_INITIALIZER;
static hipStream_t g_ks_stream = nullptr;
static uint8_t *g_ks_dev = nullptr;          /* 32 KiB arena + job array */
static const size_t KS_DEV_BYTES = 32768 + 16 * sizeof(Job);

static int ks_init_locked(void)
{
    if (g_ks_dev) return 0;
    if (tlsrec_device_check() != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    if (hipStreamCreateWithFlags(&g_ks_stream, hipStreamNonBlocking) != hipSuccess) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    if (hipMalloc((void **) &g_ks_dev, KS_DEV_BYTES) != hipSuccess) {
        g_ks_dev = nullptr;
        return TLSREC_ERR_SSL_ALLOC_FAILED;
    }
    return 0;
}

/* Run `stages` dependent launches; stage s runs jobs [first[s], first[s+1]).
 * Job pointers are arena offsets (tagged with bit 63) rebased to the device. */
static const uint64_t OFF = 1ull << 62;
static inline const uint8_t *dev_off(size_t off) { return (const uint8_t *) (uintptr_t) (OFF | off); }

static int run_jobs(Arena &ar, Job *jobs, const int *first, int stages, const size_t *outs, void *const *host_out,
                    const size_t *out_len, int nouts)
{
    pthread_mutex_lock(&g_ks_mu);
    int r = ks_init_locked();
    if (r == 0) {
        const int njobs = first[stages];
        auto fix = [](const uint8_t *p) -> const uint8_t * {
            const uint64_t v = (uint64_t) (uintptr_t) p;
            return (v & OFF) ? g_ks_dev + (v & ~OFF) : p;
        };
        for (int i = 0; i < njobs; i++) {
            jobs[i].key = fix(jobs[i].key);
            jobs[i].msg = fix(jobs[i].msg);
            jobs[i].msg2 = fix(jobs[i].msg2);
            jobs[i].out = (uint8_t *) fix(jobs[i].out);
        }
        Job *djobs = (Job *) (g_ks_dev + 32768);
        hipError_t e = hipMemcpyAsync(g_ks_dev, ar.host, ar.used, hipMemcpyHostToDevice, g_ks_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(djobs, jobs, sizeof(Job) * njobs, hipMemcpyHostToDevice, g_ks_stream);
        for (int s = 0; s < stages && e == hipSuccess; s++) {
            const uint32_t n = (uint32_t) (first[s + 1] - first[s]);
            hipLaunchKernelGGL(kdf_job_kernel, dim3(1), dim3(64), 0, g_ks_stream, djobs + first[s], n);
            e = hipGetLastError();
        }
        for (int o = 0; o < nouts && e == hipSuccess; o++)
            e = hipMemcpyAsync(host_out[o], g_ks_dev + outs[o], out_len[o], hipMemcpyDeviceToHost, g_ks_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_ks_stream);
        /* wipe secrets from the device arena (ssl_tls13_keys.c zeroizes its temporaries) */
        hipMemsetAsync(g_ks_dev, 0, ar.used, g_ks_stream);
        hipStreamSynchronize(g_ks_stream);
        if (e != hipSuccess) r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    pthread_mutex_unlock(&g_ks_mu);
    memset(ar.host, 0, ar.used);
    return r;
}

static Job job(uint32_t op, int alg, size_t key, uint32_t key_len, size_t msg, uint32_t msg_len, size_t out,
               uint32_t out_len)
{
    Job j;
    memset(&j, 0, sizeof(j));
    j.op = op;
    j.alg = (uint32_t) alg;
    j.key = dev_off(key);
    j.key_len = key_len;
    j.msg = dev_off(msg);
    j.msg_len = msg_len;
    j.msg2 = dev_off(0);
    j.msg2_len = 0;
    j.out = (uint8_t *) dev_off(out);
    j.out_len = out_len;
    return j;
}

extern "C" int tlsrec_tls13_hkdf_expand_label(int hash_alg, const unsigned char *secret, size_t secret_len,
                                              const unsigned char *label, size_t label_len,
                                              const unsigned char *ctx, size_t ctx_len, unsigned char *buf,
                                              size_t buf_len)
{
    /* argument checks in the order of ssl_tls13_keys.c:152-171 */
    if (label_len > MAX_LABEL) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (ctx_len > MAX_CONTEXT) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (buf_len > MAX_EXPANSION) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (buf_len > 255 * alg_len(a)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;   /* HKDF-Expand limit (PSA: INVALID_ARGUMENT) */
    if (secret_len > 4096) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (buf_len == 0) return 0;
    Arena ar;
    uint8_t info[2 + 1 + 6 + 249 + 1 + 64];
    const size_t il = encode_label(buf_len, label, label_len, ctx, ctx_len, info);
    const size_t o_sec = ar.put(secret, secret_len), o_info = ar.put(info, il), o_out = ar.put(nullptr, buf_len);
    memset(info, 0, sizeof(info));
    if (ar.used > 32768) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Job j[1] = { job(OP_EXPAND, a, o_sec, (uint32_t) secret_len, o_info, (uint32_t) il, o_out, (uint32_t) buf_len) };
    const int first[2] = { 0, 1 };
    void *ho[1] = { buf };
    return run_jobs(ar, j, first, 1, &o_out, ho, &buf_len, 1);
}

/* Derive-Secret with the context hashed on the device: HASH(ctx) -> EXPAND
 * with info = HkdfLabel prefix || Hash(ctx). */
static int derive_secret_impl(int a, const unsigned char *secret, size_t secret_len, const unsigned char *label,
                              size_t label_len, const unsigned char *ctx, size_t ctx_len, int ctx_hashed,
                              unsigned char *dst, size_t dst_len)
{
    if (label_len > MAX_LABEL) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (ctx_hashed != TLSREC_TLS13_CONTEXT_UNHASHED && ctx_len > MAX_CONTEXT) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (dst_len > MAX_EXPANSION) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (dst_len > 255 * alg_len(a)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (secret_len > 4096 || (ctx_hashed == TLSREC_TLS13_CONTEXT_UNHASHED && ctx_len > 16384))
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (dst_len == 0) return 0;
    Arena ar;
    const size_t H = alg_len(a);
    uint8_t info[2 + 1 + 6 + 249 + 1 + 64];
    const size_t ctx_out = ctx_hashed == TLSREC_TLS13_CONTEXT_UNHASHED ? H : ctx_len;
    /* prefix up to and including the context-length byte */
    const size_t il = encode_label(dst_len, label, label_len, nullptr, ctx_out, info);
    const size_t o_sec = ar.put(secret, secret_len), o_info = ar.put(info, il);
    const size_t o_ctx = ar.put(ctx, ctx_len), o_hash = ar.put(nullptr, 64), o_out = ar.put(nullptr, dst_len);
    memset(info, 0, sizeof(info));
    if (ar.used > 32768) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Job j[2];
    int first[3];
    int stages;
    if (ctx_hashed == TLSREC_TLS13_CONTEXT_UNHASHED) {
        j[0] = job(OP_HASH, a, 0, 0, o_ctx, (uint32_t) ctx_len, o_hash, (uint32_t) H);
        j[1] = job(OP_EXPAND, a, o_sec, (uint32_t) secret_len, o_info, (uint32_t) il, o_out, (uint32_t) dst_len);
        j[1].msg2 = dev_off(o_hash);
        j[1].msg2_len = (uint32_t) H;
        first[0] = 0; first[1] = 1; first[2] = 2;
        stages = 2;
    } else {
        j[0] = job(OP_EXPAND, a, o_sec, (uint32_t) secret_len, o_info, (uint32_t) il, o_out, (uint32_t) dst_len);
        j[0].msg2 = dev_off(o_ctx);
        j[0].msg2_len = (uint32_t) ctx_len;
        first[0] = 0; first[1] = 1;
        stages = 1;
    }
    void *ho[1] = { dst };
    return run_jobs(ar, j, first, stages, &o_out, ho, &dst_len, 1);
}

extern "C" int tlsrec_tls13_derive_secret(int hash_alg, const unsigned char *secret, size_t secret_len,
                                          const unsigned char *label, size_t label_len, const unsigned char *ctx,
                                          size_t ctx_len, int ctx_hashed, unsigned char *dstbuf, size_t dstbuf_len)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return derive_secret_impl(a, secret, secret_len, label, label_len, ctx, ctx_len, ctx_hashed, dstbuf, dstbuf_len);
}

extern "C" int tlsrec_tls13_evolve_secret(int hash_alg, const unsigned char *secret_old, const unsigned char *input,
                                          size_t input_len, unsigned char *secret_new)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t H = alg_len(a);
    if (input_len > 16384) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Arena ar;
    uint8_t info[32];
    const size_t il = encode_label(H, (const unsigned char *) "derived", 7, nullptr, H, info);
    const size_t o_old = ar.put(secret_old, secret_old ? H : 0), o_info = ar.put(info, il);
    const size_t o_empty = ar.put(nullptr, 0), o_hash = ar.put(nullptr, 64), o_tmp = ar.put(nullptr, 64);
    const bool have_in = input != NULL && input_len != 0;
    const size_t o_in = ar.put(have_in ? input : nullptr, have_in ? input_len : H);   /* zeros when absent */
    const size_t o_out = ar.put(nullptr, 64);
    Job j[3];
    int first[4];
    int stages = 0, k = 0;
    first[0] = 0;
    if (secret_old) {
        /* Derive-Secret(secret_old, "derived", "") -> tmp (ssl_tls13_keys.c:358-369) */
        j[k++] = job(OP_HASH, a, 0, 0, o_empty, 0, o_hash, (uint32_t) H);
        first[++stages] = k;
        j[k] = job(OP_EXPAND, a, o_old, (uint32_t) H, o_info, (uint32_t) il, o_tmp, (uint32_t) H);
        j[k].msg2 = dev_off(o_hash);
        j[k++].msg2_len = (uint32_t) H;
        first[++stages] = k;
    }
    /* HKDF-Extract(salt = tmp (zeros for the first stage), IKM) */
    j[k++] = job(OP_HMAC, a, o_tmp, (uint32_t) H, o_in, (uint32_t) (have_in ? input_len : H), o_out, (uint32_t) H);
    first[++stages] = k;
    void *ho[1] = { secret_new };
    return run_jobs(ar, j, first, stages, &o_out, ho, &H, 1);
}

extern "C" int tlsrec_tls13_make_traffic_keys(int hash_alg, const unsigned char *client_secret,
                                              const unsigned char *server_secret, size_t secret_len, size_t key_len,
                                              size_t iv_len, tlsrec_key_set *keys)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!keys || key_len > sizeof(keys->client_write_key) || iv_len > sizeof(keys->client_write_iv))
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (secret_len > 4096) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Arena ar;
    uint8_t ik[32], iv[32];
    const size_t lk = encode_label(key_len, (const unsigned char *) "key", 3, nullptr, 0, ik);
    const size_t lv = encode_label(iv_len, (const unsigned char *) "iv", 2, nullptr, 0, iv);
    const size_t o_c = ar.put(client_secret, secret_len), o_s = ar.put(server_secret, secret_len);
    const size_t o_ik = ar.put(ik, lk), o_iv = ar.put(iv, lv);
    const size_t o_ck = ar.put(nullptr, 32), o_ci = ar.put(nullptr, 16), o_sk = ar.put(nullptr, 32),
                 o_si = ar.put(nullptr, 16);
    Job j[4] = { job(OP_EXPAND, a, o_c, (uint32_t) secret_len, o_ik, (uint32_t) lk, o_ck, (uint32_t) key_len),
                 job(OP_EXPAND, a, o_c, (uint32_t) secret_len, o_iv, (uint32_t) lv, o_ci, (uint32_t) iv_len),
                 job(OP_EXPAND, a, o_s, (uint32_t) secret_len, o_ik, (uint32_t) lk, o_sk, (uint32_t) key_len),
                 job(OP_EXPAND, a, o_s, (uint32_t) secret_len, o_iv, (uint32_t) lv, o_si, (uint32_t) iv_len) };
    const int first[2] = { 0, 4 };
    const size_t outs[4] = { o_ck, o_ci, o_sk, o_si };
    void *ho[4] = { keys->client_write_key, keys->client_write_iv, keys->server_write_key, keys->server_write_iv };
    const size_t ol[4] = { key_len, iv_len, key_len, iv_len };
    int r = run_jobs(ar, j, first, 1, outs, ho, ol, 4);
    if (r == 0) {
        keys->key_len = key_len;
        keys->iv_len = iv_len;
    }
    return r;
}

extern "C" int tlsrec_tls13_exporter(int hash_alg, const unsigned char *secret, size_t secret_len,
                                     const unsigned char *label, size_t label_len,
                                     const unsigned char *context_value, size_t context_len, unsigned char *out,
                                     size_t out_len)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t H = alg_len(a);
    uint8_t s[64];
    /* ssl_tls13_keys.c:1836-1852: two Derive-Secret steps, unhashed contexts */
    int r = derive_secret_impl(a, secret, secret_len, label, label_len, nullptr, 0, TLSREC_TLS13_CONTEXT_UNHASHED,
                               s, H);
    if (r == 0)
        r = derive_secret_impl(a, s, H, (const unsigned char *) "exporter", 8, context_value, context_len,
                               TLSREC_TLS13_CONTEXT_UNHASHED, out, out_len);
    volatile uint8_t *v = s;
    for (size_t i = 0; i < sizeof(s); i++) v[i] = 0;
    return r;
}

extern "C" int tlsrec_tls13_update_traffic_secret(int hash_alg, const unsigned char *secret, unsigned char *next)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t H = alg_len(a);
    return tlsrec_tls13_hkdf_expand_label(hash_alg, secret, H, (const unsigned char *) "traffic upd", 11, nullptr, 0,
                                          next, H);
}

/* engine.hip: key-table bookkeeping + key setup of slots whose material was
 * written to the table's device staging area by a kernel */
extern "C" tlsrec_key_material *tlsrec__keytab_stage(tlsrec_keytab *kt);
extern "C" int tlsrec__keytab_commit_staged(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                            hipStream_t st);

/* The derive kernel alone: key material of `count` slots into the staging
 * area, nothing committed (tools/bench_keysched.py times it apart from the
 * key setup; tlsrec_tls13_keytab_derive is this + the commit). */
extern "C" int tlsrec__tls13_stage_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                        tlsrec_tls13_secret *secrets, int key_update, void *stream)
{
    if (!kt || (!secrets && count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (first > tlsrec_keytab_capacity(kt) || count > tlsrec_keytab_capacity(kt) - first)
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    uint32_t key_len, alg;
    /* TLS 1.3 suites fix the hash with the AEAD (RFC 8446 B.4):
     * TLS_AES_256_GCM_SHA384, every other suite SHA-256 */
    key_len = tlsrec_cipher_keylen(cipher);
    if (key_len == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    alg = cipher == TLSREC_CIPHER_AES_256_GCM ? H_SHA384 : H_SHA256;
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    uint8_t infos[96];
    const uint32_t H = (uint32_t) alg_len((int) alg);
    const size_t lu = encode_label(H, (const unsigned char *) "traffic upd", 11, nullptr, 0, infos);
    const size_t lk = encode_label(key_len, (const unsigned char *) "key", 3, nullptr, 0, infos + lu);
    const size_t lv = encode_label(12, (const unsigned char *) "iv", 2, nullptr, 0, infos + lu + lk);
    DeriveArgs a;
    a.secrets = secrets;
    a.out = tlsrec__keytab_stage(kt) + first;
    memcpy(a.infos, infos, sizeof(a.infos));
    a.len_upd = (uint32_t) lu;
    a.len_key = (uint32_t) lk;
    a.len_iv = (uint32_t) lv;
    a.count = count;
    a.alg = alg;
    a.cipher = (uint32_t) cipher;
    a.key_len = key_len;
    a.update = key_update ? 1u : 0u;
    hipLaunchKernelGGL(tls13_derive_kernel, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls13_keytab_derive(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                          tlsrec_tls13_secret *secrets, int key_update, void *stream)
{
    int r = tlsrec__tls13_stage_keys(kt, first, count, cipher, secrets, key_update, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, count, cipher, (hipStream_t) stream);
    return r;
}

/* ---- the rest of the ladder, single-shot (ssl_tls13_keys.c:421-650, :697, :832) ----
 * Compositions of the calls above on the kdf_job_kernel path. */
static int ladder_alg(int hash_alg, int *a)
{
    /* the reference's "!PSA_ALG_IS_HASH(hash_alg)" assertion, then the hashes this library has */
    if (((uint32_t) hash_alg & 0x7f000000u) != 0x02000000u) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    *a = alg_index(hash_alg);
    return *a < 0 ? TLSREC_ERR_SSL_BAD_INPUT_DATA : 0;
}

static int ladder_derive(int a, const unsigned char *secret, const char *label, const unsigned char *transcript,
                         size_t transcript_len, unsigned char *dst)
{
    return derive_secret_impl(a, secret, alg_len(a), (const unsigned char *) label, strlen(label), transcript,
                              transcript_len, TLSREC_TLS13_CONTEXT_HASHED, dst, alg_len(a));
}

extern "C" int tlsrec_tls13_derive_early_secrets(int hash_alg, const unsigned char *early_secret,
                                                 const unsigned char *transcript, size_t transcript_len,
                                                 tlsrec_tls13_early_secrets *derived)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!early_secret || !derived || (!transcript && transcript_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    r = ladder_derive(a, early_secret, "c e traffic", transcript, transcript_len, derived->client_early_traffic_secret);
    if (r == 0)
        r = ladder_derive(a, early_secret, "e exp master", transcript, transcript_len,
                          derived->early_exporter_master_secret);
    return r;
}

extern "C" int tlsrec_tls13_derive_handshake_secrets(int hash_alg, const unsigned char *handshake_secret,
                                                     const unsigned char *transcript, size_t transcript_len,
                                                     tlsrec_tls13_handshake_secrets *derived)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!handshake_secret || !derived || (!transcript && transcript_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    r = ladder_derive(a, handshake_secret, "c hs traffic", transcript, transcript_len,
                      derived->client_handshake_traffic_secret);
    if (r == 0)
        r = ladder_derive(a, handshake_secret, "s hs traffic", transcript, transcript_len,
                          derived->server_handshake_traffic_secret);
    return r;
}

extern "C" int tlsrec_tls13_derive_application_secrets(int hash_alg, const unsigned char *application_secret,
                                                       const unsigned char *transcript, size_t transcript_len,
                                                       tlsrec_tls13_application_secrets *derived)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!application_secret || !derived || (!transcript && transcript_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    r = ladder_derive(a, application_secret, "c ap traffic", transcript, transcript_len,
                      derived->client_application_traffic_secret_N);
    if (r == 0)
        r = ladder_derive(a, application_secret, "s ap traffic", transcript, transcript_len,
                          derived->server_application_traffic_secret_N);
    if (r == 0)
        r = ladder_derive(a, application_secret, "exp master", transcript, transcript_len,
                          derived->exporter_master_secret);
    return r;
}

extern "C" int tlsrec_tls13_derive_resumption_master_secret(int hash_alg, const unsigned char *application_secret,
                                                            const unsigned char *transcript, size_t transcript_len,
                                                            tlsrec_tls13_application_secrets *derived)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!application_secret || !derived || (!transcript && transcript_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return ladder_derive(a, application_secret, "res master", transcript, transcript_len,
                         derived->resumption_master_secret);
}

/* ssl_tls13_calc_finished_core: EXPAND "finished" -> HMAC over the transcript hash, one job chain */
static int calc_finished_impl(int a, const unsigned char *base, const unsigned char *transcript, unsigned char *dst)
{
    const size_t H = alg_len(a);
    Arena ar;
    uint8_t info[32];
    const size_t il = encode_label(H, (const unsigned char *) "finished", 8, nullptr, 0, info);
    const size_t o_base = ar.put(base, H), o_info = ar.put(info, il), o_tr = ar.put(transcript, H);
    const size_t o_key = ar.put(nullptr, 64), o_out = ar.put(nullptr, 64);
    Job j[2] = { job(OP_EXPAND, a, o_base, (uint32_t) H, o_info, (uint32_t) il, o_key, (uint32_t) H),
                 job(OP_HMAC, a, o_key, (uint32_t) H, o_tr, (uint32_t) H, o_out, (uint32_t) H) };
    const int first[3] = { 0, 1, 2 };
    void *ho[1] = { dst };
    return run_jobs(ar, j, first, 2, &o_out, ho, &H, 1);
}

extern "C" int tlsrec_tls13_calc_finished(int hash_alg, const unsigned char *base_secret,
                                          const unsigned char *transcript, unsigned char *out, size_t *out_len)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!base_secret || !transcript || !out || !out_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    r = calc_finished_impl(a, base_secret, transcript, out);
    if (r == 0) *out_len = alg_len(a);
    return r;
}

extern "C" int tlsrec_tls13_create_psk_binder(int hash_alg, const unsigned char *psk, size_t psk_len, int psk_type,
                                              const unsigned char *transcript, unsigned char *result)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if ((!psk && psk_len) || !transcript || !result) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    uint8_t early[64], binder_key[64];
    r = tlsrec_tls13_evolve_secret(hash_alg, nullptr, psk, psk_len, early);
    /* ssl_tls13_keys.c:879-895: "res binder" for a resumption PSK, "ext binder" for any other type */
    const char *lbl = psk_type == TLSREC_TLS13_PSK_RESUMPTION ? "res binder" : "ext binder";
    if (r == 0)
        r = derive_secret_impl(a, early, alg_len(a), (const unsigned char *) lbl, 10, nullptr, 0,
                               TLSREC_TLS13_CONTEXT_UNHASHED, binder_key, alg_len(a));
    if (r == 0) r = calc_finished_impl(a, binder_key, transcript, result);
    volatile uint8_t *v = early, *u = binder_key;
    for (size_t i = 0; i < 64; i++) { v[i] = 0; u[i] = 0; }
    return r;
}

/* ---- the ladder in batches (tls13_hs_kernel, tls13_app_kernel, tls13_mac_kernel) ---- */
/* HMAC midstates of the zero salt, of Derive-Secret(Extract(0, 0), "derived", ""),
 * and Hash(""): tests/tls13_ref.py ladder_constants() computes them from FIPS 180-4
 * and hashlib, tests/test_tls13_ladder_cpu.py compares. */
static const LadderConsts<L256> kConsts256 = {
    { 0xf454deadu, 0x9725214fu, 0x90daf2a0u, 0xdf1228eau, 0x64e5750fu, 0xa3924181u, 0x824a932bu, 0xf8e04e32u },
    { 0xd385480fu, 0x7abb6477u, 0x37c9c538u, 0x5dd82467u, 0x8e043a72u, 0x753434b0u, 0xdeb82818u, 0x361d45a6u },
    { 0x8b35051cu, 0x8324ce6fu, 0xd35fd442u, 0x05006b0bu, 0x11f653deu, 0x87170024u, 0x53923a72u, 0x1a2e89f5u },
    { 0x22b91d2fu, 0xa7f9ba55u, 0xba705a48u, 0xa6bef047u, 0xf5ba9b91u, 0xc425b796u, 0xdb8072a6u, 0x9037dbc2u },
    { 0xe3b0c442u, 0x98fc1c14u, 0x9afbf4c8u, 0x996fb924u, 0x27ae41e4u, 0x649b934cu, 0xa495991bu, 0x7852b855u } };
static const LadderConsts<L384> kConsts384 = {
    { 0x53f869327560c3a2ULL, 0xc237b05164a5bbe8ULL, 0xe581f7394cfa66b8ULL, 0x846fa61922faad62ULL,
      0xdd0b37ce462cff5eULL, 0x7ee8a4bdc87567f3ULL, 0x39bda99c75a047f7ULL, 0xc7bd628bd3f9a734ULL },
    { 0xff6ce3f9ca86c81cULL, 0x585559c2ae0fc15cULL, 0xcf0d5686fb65a54eULL, 0xf1d54ee19e8cfd02ULL,
      0xa5c720ab778ff100ULL, 0xdeb3e5f667573e8cULL, 0xc1bfc7ec16b591f3ULL, 0x34d487c1c79d59ebULL },
    { 0x9540faa284271b10ULL, 0x940f9b21f2567a8cULL, 0x43d6380a7b89a867ULL, 0xedb7635f9865feb1ULL,
      0x7c8b33059f3e823eULL, 0x9eb66f676065f021ULL, 0x79f7d919bede4e6dULL, 0x80ad994f8a39c726ULL },
    { 0x9dcd6bc600f811e3ULL, 0xc556680dbba9586eULL, 0x987fb78efb62dcb7ULL, 0xb639835d0b42573aULL,
      0x81cf02b2e173ad99ULL, 0x30a7f1029298d495ULL, 0x8aa72679937f7672ULL, 0xd31f72c4ad9a4b4cULL },
    { 0x38b060a751ac9638ULL, 0x4cd9327eb1b1e36aULL, 0x21fdb71114be0743ULL, 0x4c0cc7bf63f6e1daULL,
      0x274edebfe76f65fbULL, 0xd51ad2f14898b95bULL } };

template <class T> static const LadderConsts<T> &ladder_consts();
template <> const LadderConsts<L256> &ladder_consts<L256>() { return kConsts256; }
template <> const LadderConsts<L384> &ladder_consts<L384>() { return kConsts384; }

/* Host-only: the constants of `hash_alg` widened to 64 bits, zero_ip | zero_op |
 * d0_ip | d0_op | empty (40 words for SHA-256, 38 for SHA-384); returns the count. */
extern "C" int tlsrec__tls13_ladder_consts(int hash_alg, uint64_t *out)
{
    const int a = alg_index(hash_alg);
    if (a < 0 || !out) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    int n = 0;
    if (a == H_SHA384) {
        const LadderConsts<L384> &k = kConsts384;
        for (int j = 0; j < 8; j++) out[n++] = k.zero_ip[j];
        for (int j = 0; j < 8; j++) out[n++] = k.zero_op[j];
        for (int j = 0; j < 8; j++) out[n++] = k.d0_ip[j];
        for (int j = 0; j < 8; j++) out[n++] = k.d0_op[j];
        for (int j = 0; j < L384::HW; j++) out[n++] = k.empty[j];
    } else {
        const LadderConsts<L256> &k = kConsts256;
        for (int j = 0; j < 8; j++) out[n++] = k.zero_ip[j];
        for (int j = 0; j < 8; j++) out[n++] = k.zero_op[j];
        for (int j = 0; j < 8; j++) out[n++] = k.d0_ip[j];
        for (int j = 0; j < 8; j++) out[n++] = k.d0_op[j];
        for (int j = 0; j < L256::HW; j++) out[n++] = k.empty[j];
    }
    return n;
}

/* Host-only: the inner message of the exporter's first step (ssl_tls13_keys.c:1838),
 * HkdfLabel(H, label, Hash("")) || 0x01, the same for every connection of a call:
 * 11 + label_len + H bytes, padded as the blocks after an HMAC's ipad block (0x80,
 * zeros, the length (BB + n) * 8) into big-endian words widened to 64 bits, 16 a
 * block; *nblk blocks, at most 5 (SHA-256) or 3 (SHA-384).  words_out holds 80. */
extern "C" int tlsrec__tls13_exporter_blocks(int hash_alg, const unsigned char *label, size_t label_len,
                                             uint64_t *words_out, uint32_t *nblk)
{
    const int a = alg_index(hash_alg);
    if (a < 0 || !words_out || !nblk || (!label && label_len) || label_len > MAX_LABEL)
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t H = alg_len(a), BB = a == H_SHA384 ? 128 : 64, LENB = BB / 8, wb = BB / 16;
    uint8_t e[48], m[5 * 64 + 128] = { 0 };
    for (size_t j = 0; j < H; j++) {
        e[j] = a == H_SHA384 ? (uint8_t) (kConsts384.empty[j / 8] >> (56 - 8 * (j % 8)))
                             : (uint8_t) (kConsts256.empty[j / 4] >> (24 - 8 * (j % 4)));
    }
    size_t n = encode_label(H, label, label_len, e, H, m);
    m[n++] = 0x01;
    const size_t blocks = (n + 1 + LENB + BB - 1) / BB;
    const uint64_t bits = (uint64_t) (BB + n) * 8;
    m[n] = 0x80;
    for (size_t j = 0; j < 8; j++) m[blocks * BB - 1 - j] = (uint8_t) (bits >> (8 * j));
    for (size_t k = 0; k < 16 * blocks; k++) {
        uint64_t v = 0;
        for (size_t j = 0; j < wb; j++) v = (v << 8) | m[k * wb + j];
        words_out[k] = v;
    }
    *nblk = (uint32_t) blocks;
    return 0;
}

/* HkdfLabel(desired, label, context of ctx_len bytes to follow) as the kernels' cells */
static LabelW label_cells(size_t desired, const void *label, size_t label_len, size_t ctx_len)
{
    uint8_t b[24] = { 0 };
    encode_label(desired, (const unsigned char *) label, label_len, nullptr, ctx_len, b);
    LabelW l;
    for (int c = 0; c < 6; c++)
        l.c[c] = ((uint32_t) b[4 * c] << 24) | ((uint32_t) b[4 * c + 1] << 16) | ((uint32_t) b[4 * c + 2] << 8) | b[4 * c + 3];
    return l;
}

static LadderLabels ladder_labels(size_t H, size_t key_len, const char *c_traffic, const char *s_traffic,
                                  const char *extra)
{
    LadderLabels lb;
    lb.derived = label_cells(H, "derived", 7, H);
    lb.c_traffic = label_cells(H, c_traffic, 12, H);
    lb.s_traffic = label_cells(H, s_traffic, 12, H);
    lb.extra = label_cells(H, extra, strlen(extra), H);
    lb.key = label_cells(key_len, "key", 3, 0);
    lb.iv = label_cells(12, "iv", 2, 0);
    lb.fin = label_cells(H, "finished", 8, 0);
    return lb;
}

static inline uint32_t al(const void *p, uint32_t bit) { return ((uintptr_t) p & 15) == 0 ? bit : 0u; }

/* the checks the two stages share, in the header's order; *alg: the suite's hash as in tlsrec_tls13_keytab_derive */
static int ladder_check(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, bool null_array, uint32_t psk_len,
                        uint32_t shared_len, int *alg)
{
    if (!kt || (null_array && count) || psk_len > 48) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const uint32_t cap = tlsrec_keytab_capacity(kt);
    if (first > cap || (uint64_t) count * 2 > (uint64_t) (cap - first)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (tlsrec_cipher_keylen(cipher) == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (shared_len != 0 && shared_len != 32 && shared_len != 48 && shared_len != 56 && shared_len != 66)
        return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    *alg = cipher == TLSREC_CIPHER_AES_256_GCM ? H_SHA384 : H_SHA256;
    return 0;
}

static uint32_t tls13_head(int cipher)
{
    /* tlsrec_key_material: cipher, tls_minor 4, fixed_ivlen 12 (ssl_tls13_keys.c:985-998), taglen */
    return (uint32_t) cipher | (4u << 8) | (12u << 16) | ((uint32_t) tlsrec_cipher_taglen(cipher) << 24);
}

template <class T>
static hipError_t hs_launch(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, uint32_t psk_len,
                            uint32_t shared_len, const tlsrec_tls13_hs_conn *conns, tlsrec_tls13_secret *hs_traffic,
                            tlsrec_tls13_secret *finished_keys, tlsrec_tls13_secret *master, hipStream_t st)
{
    Tls13HsArgs<T> a;
    a.conns = conns;
    a.out = tlsrec__keytab_stage(kt) + first;
    a.hs_traffic = hs_traffic;
    a.finished = finished_keys;
    a.master = master;
    a.count = count;
    a.head = tls13_head(cipher);
    a.key_cells = tlsrec_cipher_keylen(cipher) / 4;
    a.psk_len = psk_len;
    a.shared_len = shared_len;
    a.aligned = al(conns, AL_CONNS) | al(hs_traffic, AL_TRAFFIC) | al(finished_keys, AL_AUX) | al(master, AL_MASTER);
    a.k = ladder_consts<T>();
    a.lb = ladder_labels(T::HB, tlsrec_cipher_keylen(cipher), "c hs traffic", "s hs traffic", "");
    hipLaunchKernelGGL(tls13_hs_kernel<T>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

/* The derive kernel alone (see tlsrec__tls13_stage_keys). */
extern "C" int tlsrec__tls13_stage_hs_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                           uint32_t psk_len, uint32_t shared_len, const tlsrec_tls13_hs_conn *conns,
                                           tlsrec_tls13_secret *hs_traffic, tlsrec_tls13_secret *finished_keys,
                                           tlsrec_tls13_secret *master, void *stream)
{
    int alg;
    int r = ladder_check(kt, first, count, cipher, !conns || !hs_traffic || !master, psk_len, shared_len, &alg);
    if (r != 0 || count == 0) return r;
    hipStream_t st = (hipStream_t) stream;
    const hipError_t e = alg == H_SHA384
        ? hs_launch<L384>(kt, first, count, cipher, psk_len, shared_len, conns, hs_traffic, finished_keys, master, st)
        : hs_launch<L256>(kt, first, count, cipher, psk_len, shared_len, conns, hs_traffic, finished_keys, master, st);
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls13_keytab_derive_handshake(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                                    uint32_t psk_len, uint32_t shared_len,
                                                    const tlsrec_tls13_hs_conn *conns, tlsrec_tls13_secret *hs_traffic,
                                                    tlsrec_tls13_secret *finished_keys, tlsrec_tls13_secret *master,
                                                    void *stream)
{
    int r = tlsrec__tls13_stage_hs_keys(kt, first, count, cipher, psk_len, shared_len, conns, hs_traffic, finished_keys,
                                        master, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, 2 * count, cipher, (hipStream_t) stream);
    return r;
}

template <class T>
static hipError_t app_launch(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                             const tlsrec_tls13_secret *master, const tlsrec_tls13_secret *transcripts,
                             tlsrec_tls13_secret *app_traffic, tlsrec_tls13_secret *exporter, hipStream_t st)
{
    Tls13AppArgs<T> a;
    a.master = master;
    a.transcripts = transcripts;
    a.out = tlsrec__keytab_stage(kt) + first;
    a.app_traffic = app_traffic;
    a.exporter = exporter;
    a.count = count;
    a.head = tls13_head(cipher);
    a.key_cells = tlsrec_cipher_keylen(cipher) / 4;
    a.aligned = al(master, AL_MASTER) | al(transcripts, AL_TRANSCRIPT) | al(app_traffic, AL_TRAFFIC) | al(exporter, AL_AUX);
    a.lb = ladder_labels(T::HB, tlsrec_cipher_keylen(cipher), "c ap traffic", "s ap traffic", "exp master");
    hipLaunchKernelGGL(tls13_app_kernel<T>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

extern "C" int tlsrec__tls13_stage_app_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                            const tlsrec_tls13_secret *master, const tlsrec_tls13_secret *transcripts,
                                            tlsrec_tls13_secret *app_traffic, tlsrec_tls13_secret *exporter, void *stream)
{
    int alg;
    int r = ladder_check(kt, first, count, cipher, !master || !transcripts || !app_traffic, 0, 0, &alg);
    if (r != 0 || count == 0) return r;
    hipStream_t st = (hipStream_t) stream;
    const hipError_t e = alg == H_SHA384
        ? app_launch<L384>(kt, first, count, cipher, master, transcripts, app_traffic, exporter, st)
        : app_launch<L256>(kt, first, count, cipher, master, transcripts, app_traffic, exporter, st);
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls13_keytab_derive_application(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                                      const tlsrec_tls13_secret *master,
                                                      const tlsrec_tls13_secret *transcripts,
                                                      tlsrec_tls13_secret *app_traffic, tlsrec_tls13_secret *exporter,
                                                      void *stream)
{
    int r = tlsrec__tls13_stage_app_keys(kt, first, count, cipher, master, transcripts, app_traffic, exporter, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, 2 * count, cipher, (hipStream_t) stream);
    return r;
}

static int mac_launch(int hash_alg, uint32_t label_len, const unsigned char *label, const tlsrec_tls13_secret *keys,
                      const tlsrec_tls13_secret *msgs, tlsrec_tls13_secret *out, uint32_t count, void *stream)
{
    const int alg = alg_index(hash_alg);
    if (alg < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if ((!keys || !msgs || !out) && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    static const int device = tlsrec_device_check();     /* no key table vouches for a device here; asked once */
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls13MacArgs a;
    a.keys = keys;
    a.msgs = msgs;
    a.out = out;
    a.count = count;
    a.aligned = al(keys, AL_MASTER) | al(msgs, AL_TRANSCRIPT) | al(out, AL_AUX);
    a.label_len = label_len;
    memset(&a.label, 0, sizeof(a.label));
    if (label_len != MAC_PLAIN) a.label = label_cells(alg_len(alg), label, label_len, alg_len(alg));
    hipStream_t st = (hipStream_t) stream;
    if (alg == H_SHA384) hipLaunchKernelGGL(tls13_mac_kernel<L384>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(tls13_mac_kernel<L256>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls13_batch_verify_data(int hash_alg, const tlsrec_tls13_secret *finished_keys,
                                              const tlsrec_tls13_secret *transcripts, tlsrec_tls13_secret *out,
                                              uint32_t count, void *stream)
{
    return mac_launch(hash_alg, MAC_PLAIN, nullptr, finished_keys, transcripts, out, count, stream);
}

extern "C" int tlsrec_tls13_batch_derive_secret(int hash_alg, const unsigned char *label, size_t label_len,
                                                const tlsrec_tls13_secret *secrets, const tlsrec_tls13_secret *transcripts,
                                                tlsrec_tls13_secret *out, uint32_t count, void *stream)
{
    if (label_len > 12 || (!label && label_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return mac_launch(hash_alg, (uint32_t) label_len, label, secrets, transcripts, out, count, stream);
}

/* ---- keying material exporters in batches (tls13_exporter_kernel, tls12_export_kernel) ---- */
static const uint32_t EXPORT_MAX_KEY_LEN = 8160;     /* MBEDTLS_SSL_EXPORT_MAX_KEY_LEN, ssl.h */
static const uint32_t EXPORT_MAX_CONTEXT = 255;      /* the batch form's limit: longer contexts stay single-shot */

/* the checks the two exporter batches share, in the header's order, after the hash / PRF; `ctx`: a context is used */
static int export_check(const void *in, const void *contexts, const void *out, const void *label, size_t label_len,
                        bool ctx, uint32_t context_len, uint32_t context_stride, uint32_t out_len, uint32_t out_stride,
                        uint32_t count)
{
    if (count && (!in || !out || (!contexts && ctx && context_len))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!label && label_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (label_len > MAX_LABEL) return TLSREC_ERR_SSL_BAD_INPUT_DATA;                      /* ssl_tls.c:8959 */
    if (out_len > EXPORT_MAX_KEY_LEN) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (out_stride < out_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (ctx && context_stride != 0 && context_stride < context_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (ctx && context_len > EXPORT_MAX_CONTEXT) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    return 0;
}

/* 16-byte stores need the base and the stride aligned */
static inline uint32_t al_out(const void *out, uint32_t stride) { return (stride & 15) == 0 ? al(out, AL_OUT) : 0u; }

template <class T>
static hipError_t exporter_launch(const tlsrec_tls13_secret *secrets, const unsigned char *label, size_t label_len,
                                  const uint8_t *contexts, uint32_t context_len, uint32_t context_stride, uint8_t *out,
                                  uint32_t out_len, uint32_t out_stride, uint32_t count, int hash_alg, hipStream_t st)
{
    Tls13ExporterArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.secrets = secrets;
    a.contexts = contexts;
    a.out = out;
    a.count = count;
    a.context_len = context_len;
    a.context_stride = context_stride;
    a.out_len = out_len;
    a.out_stride = out_stride;
    a.aligned = al(secrets, AL_SECRETS) | al_out(out, out_stride);
    a.label = label_cells(out_len, "exporter", 8, T::HB);
    for (int j = 0; j < T::HW; j++) a.empty[j] = ladder_consts<T>().empty[j];
    uint64_t words[80];
    if (tlsrec__tls13_exporter_blocks(hash_alg, label, label_len, words, &a.nblk) != 0) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < 16 * a.nblk; k++) a.words[k] = (typename T::W) words[k];
    hipLaunchKernelGGL(tls13_exporter_kernel<T>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

extern "C" int tlsrec_tls13_batch_exporter(int hash_alg, const tlsrec_tls13_secret *secrets,
                                           const unsigned char *label, size_t label_len, const uint8_t *contexts,
                                           uint32_t context_len, uint32_t context_stride, uint8_t *out,
                                           uint32_t out_len, uint32_t out_stride, uint32_t count, void *stream)
{
    const int alg = alg_index(hash_alg);
    if (alg < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const int r = export_check(secrets, contexts, out, label, label_len, true, context_len, context_stride, out_len,
                               out_stride, count);
    if (r != 0 || count == 0 || out_len == 0) return r;
    static const int device = tlsrec_device_check();     /* no key table vouches for a device here; asked once */
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    const hipError_t e =
        alg == H_SHA384 ? exporter_launch<L384>(secrets, label, label_len, contexts, context_len, context_stride, out,
                                                out_len, out_stride, count, hash_alg, (hipStream_t) stream)
                        : exporter_launch<L256>(secrets, label, label_len, contexts, context_len, context_stride, out,
                                                out_len, out_stride, count, hash_alg, (hipStream_t) stream);
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

/* ---- a resumed handshake in batches (tls13_early_kernel, tls13_ticket_kernel) ---- */
/* the BAD_INPUT_DATA checks the binder and the early-key calls share, in the header's order */
static bool early_args_bad(bool null_array, uint32_t count, const void *offered, const void *binders, const void *match,
                           uint32_t psk_len)
{
    if (null_array && count) return true;
    if ((offered == nullptr) != (match == nullptr)) return true;
    if (!binders && !match && count) return true;
    return psk_len == 0 || psk_len > 48;
}

/* kt NULL: the binder alone, nothing staged */
template <class T>
static hipError_t early_launch(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, uint32_t psk_len,
                               int psk_type, const tlsrec_tls13_psk_conn *conns, const tlsrec_tls13_secret *offered,
                               tlsrec_tls13_secret *binders, uint32_t *match, tlsrec_tls13_secret *early_traffic,
                               tlsrec_tls13_secret *early_exporter, hipStream_t st)
{
    Tls13EarlyArgs<T> a;
    a.conns = conns;
    a.offered = offered;
    a.binders = binders;
    a.match = match;
    a.out = kt ? tlsrec__keytab_stage(kt) + first : nullptr;
    a.early_traffic = early_traffic;
    a.early_exporter = early_exporter;
    a.count = count;
    a.head = kt ? tls13_head(cipher) : 0u;
    a.key_cells = kt ? tlsrec_cipher_keylen(cipher) / 4 : 0u;
    a.psk_len = psk_len;
    a.aligned = al(conns, AL_CONNS) | al(offered, AL_OFFERED) | al(binders, AL_BINDERS) | al(early_traffic, AL_TRAFFIC) |
                al(early_exporter, AL_AUX);
    a.k = ladder_consts<T>();
    /* ssl_tls13_keys.c:879-895: "res binder" for a resumption PSK, "ext binder" for any other type */
    a.binder = label_cells(T::HB, psk_type == TLSREC_TLS13_PSK_RESUMPTION ? "res binder" : "ext binder", 10, T::HB);
    a.c_e = label_cells(T::HB, "c e traffic", 11, T::HB);
    a.e_exp = label_cells(T::HB, "e exp master", 12, T::HB);
    memset(&a.lb, 0, sizeof(a.lb));
    a.lb.key = label_cells(kt ? tlsrec_cipher_keylen(cipher) : 0, "key", 3, 0);
    a.lb.iv = label_cells(12, "iv", 2, 0);
    a.lb.fin = label_cells(T::HB, "finished", 8, 0);
    hipLaunchKernelGGL(tls13_early_kernel<T>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

extern "C" int tlsrec_tls13_batch_psk_binder(int hash_alg, uint32_t psk_len, int psk_type,
                                             const tlsrec_tls13_psk_conn *conns, const tlsrec_tls13_secret *offered,
                                             tlsrec_tls13_secret *binders, uint32_t *match, uint32_t count, void *stream)
{
    const int alg = alg_index(hash_alg);
    if (alg < 0 || early_args_bad(!conns, count, offered, binders, match, psk_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    static const int device = tlsrec_device_check();     /* no key table vouches for a device here; asked once */
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    hipStream_t st = (hipStream_t) stream;
    const hipError_t e = alg == H_SHA384
        ? early_launch<L384>(nullptr, 0, count, 0, psk_len, psk_type, conns, offered, binders, match, nullptr, nullptr, st)
        : early_launch<L256>(nullptr, 0, count, 0, psk_len, psk_type, conns, offered, binders, match, nullptr, nullptr, st);
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

/* The derive kernel alone (see tlsrec__tls13_stage_keys). */
extern "C" int tlsrec__tls13_stage_early_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                              uint32_t psk_len, int psk_type, const tlsrec_tls13_psk_conn *conns,
                                              const tlsrec_tls13_secret *offered, tlsrec_tls13_secret *binders,
                                              uint32_t *match, tlsrec_tls13_secret *early_traffic,
                                              tlsrec_tls13_secret *early_exporter, void *stream)
{
    if (!kt || early_args_bad(!conns || !early_traffic, count, offered, binders, match, psk_len))
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const uint32_t cap = tlsrec_keytab_capacity(kt);
    if (first > cap || count > cap - first) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (tlsrec_cipher_keylen(cipher) == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    const hipError_t e = cipher == TLSREC_CIPHER_AES_256_GCM
        ? early_launch<L384>(kt, first, count, cipher, psk_len, psk_type, conns, offered, binders, match, early_traffic,
                             early_exporter, st)
        : early_launch<L256>(kt, first, count, cipher, psk_len, psk_type, conns, offered, binders, match, early_traffic,
                             early_exporter, st);
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls13_keytab_derive_early(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                                uint32_t psk_len, int psk_type, const tlsrec_tls13_psk_conn *conns,
                                                const tlsrec_tls13_secret *offered, tlsrec_tls13_secret *binders,
                                                uint32_t *match, tlsrec_tls13_secret *early_traffic,
                                                tlsrec_tls13_secret *early_exporter, void *stream)
{
    int r = tlsrec__tls13_stage_early_keys(kt, first, count, cipher, psk_len, psk_type, conns, offered, binders, match,
                                           early_traffic, early_exporter, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, count, cipher, (hipStream_t) stream);
    return r;
}

extern "C" int tlsrec_tls13_batch_ticket_psk(int hash_alg, uint32_t nonce_len, const tlsrec_tls13_secret *res_master,
                                             const uint8_t *nonces, tlsrec_tls13_secret *psk, uint32_t count,
                                             void *stream)
{
    const int alg = alg_index(hash_alg);
    if (alg < 0 || ((!res_master || !nonces || !psk) && count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (nonce_len > 32) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (count == 0) return 0;
    static const int device = tlsrec_device_check();
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls13TicketArgs a;
    a.res_master = res_master;
    a.nonces = nonces;
    a.psk = psk;
    a.count = count;
    a.aligned = al(res_master, AL_MASTER) | al(nonces, AL_TRANSCRIPT) | al(psk, AL_AUX);
    a.nonce_len = nonce_len;
    a.label = label_cells(alg_len(alg), "resumption", 10, nonce_len);
    hipStream_t st = (hipStream_t) stream;
    if (alg == H_SHA384) hipLaunchKernelGGL(tls13_ticket_kernel<L384>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(tls13_ticket_kernel<L256>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

/* ======================================================================
 * TLS 1.2 / DTLS 1.2 (library/ssl_tls.c)
 *
 *   reference                                        here
 *   mbedtls_ssl_tls_prf               :465           tlsrec_tls_prf
 *   tls_prf_generic                   :6099          OP_PRF (tls_prf() above)
 *   ssl_compute_master                :6251-6451     tlsrec_tls12_compute_master (non-PSK branch)
 *   key-block split                   :7858-7892     tlsrec_tls12_split_key_block (host only)
 *   tls_prf(.., "key expansion", ..)  :7750          tlsrec_tls12_make_keys
 *   mbedtls_ssl_tls12_export_keying_material :8886   tlsrec_tls12_export_keying_material
 *   (batch)                                          tlsrec_tls12_keytab_derive, _derive_cbc
 * ==================================================================== */
static int prf_index(int prf)
{
    return prf == TLSREC_TLS_PRF_SHA256 ? H_SHA256 : prf == TLSREC_TLS_PRF_SHA384 ? H_SHA384 : -1;
}

/* fixed_ivlen of a TLS 1.2 AEAD transform, ssl_tls.c:7722-7727 */
static size_t tls12_fixed_ivlen(int cipher) { return cipher == TLSREC_CIPHER_CHACHA20_POLY1305 ? 12 : 4; }

static void wipe(void *p, size_t n)
{
    volatile uint8_t *v = (volatile uint8_t *) p;
    for (size_t i = 0; i < n; i++) v[i] = 0;
}

/* PRF with seed = label || r1 || r2 through the arena (a = H_SHA256 / H_SHA384) */
static int prf_run(int a, const unsigned char *secret, size_t slen, const char *label, size_t llen,
                   const unsigned char *r1, size_t r1len, const unsigned char *r2, size_t r2len,
                   unsigned char *dst, size_t dlen)
{
    if ((slen && !secret) || (llen && !label) || (r1len && !r1) || (r2len && !r2) || !dst)
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* the arena holds the secret, the label, the random bytes and the output, each rounded to 16 bytes */
    const size_t lim = 32768;
    if (slen > lim || llen > lim || r1len > lim || r2len > lim || dlen > lim) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t rlen = r1len + r2len;
    if (((slen + 15) & ~(size_t) 15) + ((llen + 15) & ~(size_t) 15) + ((rlen + 15) & ~(size_t) 15) +
        ((dlen + 15) & ~(size_t) 15) > lim)
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Arena ar;
    const size_t o_sec = ar.put(secret, slen), o_lab = ar.put(label, llen);
    const size_t o_rnd = ar.used;
    if (r1len) memcpy(ar.host + o_rnd, r1, r1len);
    if (r2len) memcpy(ar.host + o_rnd + r1len, r2, r2len);
    ar.used = (ar.used + rlen + 15) & ~(size_t) 15;
    const size_t o_out = ar.put(nullptr, dlen);
    Job j[1] = { job(OP_PRF, a, o_sec, (uint32_t) slen, o_lab, (uint32_t) llen, o_out, (uint32_t) dlen) };
    j[0].msg2 = dev_off(o_rnd);
    j[0].msg2_len = (uint32_t) rlen;
    const int first[2] = { 0, 1 };
    void *ho[1] = { dst };
    return run_jobs(ar, j, first, 1, &o_out, ho, &dlen, 1);
}

extern "C" int tlsrec_tls_prf(int prf, const unsigned char *secret, size_t slen, const char *label,
                              const unsigned char *random, size_t rlen, unsigned char *dstbuf, size_t dlen)
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;      /* ssl_tls.c:489-490 */
    if (dlen == 0) return 0;
    if (!label) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return prf_run(a, secret, slen, label, strlen(label), random, rlen, nullptr, 0, dstbuf, dlen);
}

extern "C" int tlsrec_tls12_compute_master(int prf, const unsigned char *premaster, size_t pmslen,
                                           const unsigned char *seed, size_t seed_len, int extended_ms,
                                           unsigned char master[48])
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    /* ssl_tls.c:6269, :6295 */
    const char *lbl = extended_ms ? "extended master secret" : "master secret";
    return prf_run(a, premaster, pmslen, lbl, strlen(lbl), seed, seed_len, nullptr, 0, master, 48);
}

extern "C" int tlsrec_tls12_split_key_block(int cipher, const unsigned char *keyblk, size_t keyblk_len,
                                            tlsrec_key_set *keys)
{
    if (!keys || !keyblk) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t kl = tlsrec_cipher_keylen(cipher);
    if (kl == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    const size_t il = tls12_fixed_ivlen(cipher);
    if (keyblk_len < 2 * kl + 2 * il) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    memset(keys, 0, sizeof(*keys));
    /* ssl_tls.c:7858-7892 with mac_key_len = 0: key1 = keyblk, key2 = key1 + keylen,
     * the IVs follow; the client writes with key1 / the first IV */
    memcpy(keys->client_write_key, keyblk, kl);
    memcpy(keys->server_write_key, keyblk + kl, kl);
    memcpy(keys->client_write_iv, keyblk + 2 * kl, il);
    memcpy(keys->server_write_iv, keyblk + 2 * kl + il, il);
    keys->key_len = kl;
    keys->iv_len = il;
    return 0;
}

extern "C" int tlsrec_tls12_make_keys(int prf, int cipher, const unsigned char master[48],
                                      const unsigned char randbytes[64], tlsrec_key_set *keys)
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    const size_t kl = tlsrec_cipher_keylen(cipher);
    if (kl == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (!master || !randbytes || !keys) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* the reference expands 256 bytes (ssl_tls.c:7750) and uses this prefix of them */
    unsigned char keyblk[96];
    const size_t need = 2 * kl + 2 * tls12_fixed_ivlen(cipher);
    int r = prf_run(a, master, 48, "key expansion", 13, randbytes, 64, nullptr, 0, keyblk, need);
    if (r == 0) r = tlsrec_tls12_split_key_block(cipher, keyblk, need, keys);
    wipe(keyblk, sizeof(keyblk));
    return r;
}

/* the CBC + HMAC suites' layout (mac_key_len != 0), ssl_tls.c:7858-7886:
 * client_mac | server_mac | client_key | server_key (TLS 1.2 carries the CBC
 * IV in each record, so the IV part of the block goes unused) */
static size_t cbc_split_keylen(int cipher)
{
    switch (cipher) {
        case TLSREC_CIPHER_AES_128_CBC: case TLSREC_CIPHER_ARIA_128_CBC: case TLSREC_CIPHER_CAMELLIA_128_CBC: return 16;
        case TLSREC_CIPHER_AES_256_CBC: case TLSREC_CIPHER_ARIA_256_CBC: case TLSREC_CIPHER_CAMELLIA_256_CBC: return 32;
        default: return 0;
    }
}
static size_t cbc_split_maclen(int mac)
{
    return mac == TLSREC_MAC_SHA1 ? 20 : mac == TLSREC_MAC_SHA256 ? 32 : mac == TLSREC_MAC_SHA384 ? 48 : 0;
}
/* a pair tlsrec_keytab_load_cbc takes: AES with every MAC, an ARIA / Camellia id
 * only with its suites' MAC (128-bit keys SHA-256, 256-bit keys SHA-384) */
static bool cbc_split_pair_ok(int cipher, int mac)
{
    const size_t kl = cbc_split_keylen(cipher), ml = cbc_split_maclen(mac);
    if (kl == 0 || ml == 0) return false;
    if (cipher <= TLSREC_CIPHER_AES_256_CBC) return true;
    return mac == (kl == 16 ? TLSREC_MAC_SHA256 : TLSREC_MAC_SHA384);
}

extern "C" int tlsrec_tls12_split_key_block_cbc(int cipher, int mac, const unsigned char *keyblk, size_t keyblk_len,
                                                tlsrec_cbc_key_set *out)
{
    if (!out || !keyblk) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t kl = cbc_split_keylen(cipher), ml = cbc_split_maclen(mac);
    if (!cbc_split_pair_ok(cipher, mac)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (keyblk_len < 2 * ml + 2 * kl) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    memset(out, 0, sizeof(*out));
    tlsrec_cbc_key_material *dir[2] = { &out->client_write, &out->server_write };
    for (int i = 0; i < 2; i++) {
        dir[i]->cipher = (uint8_t) cipher;
        dir[i]->tls_minor = 3;
        dir[i]->mac = (uint8_t) mac;
        memcpy(dir[i]->mac_key, keyblk + i * ml, ml);
        memcpy(dir[i]->key, keyblk + 2 * ml + i * kl, kl);
    }
    return 0;
}

extern "C" int tlsrec_tls12_make_keys_cbc(int prf, int cipher, int mac, const unsigned char master[48],
                                          const unsigned char randbytes[64], tlsrec_cbc_key_set *out)
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    const size_t kl = cbc_split_keylen(cipher), ml = cbc_split_maclen(mac);
    if (!cbc_split_pair_ok(cipher, mac)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (!master || !randbytes || !out) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    unsigned char keyblk[160];
    const size_t need = 2 * ml + 2 * kl;
    int r = prf_run(a, master, 48, "key expansion", 13, randbytes, 64, nullptr, 0, keyblk, need);
    if (r == 0) r = tlsrec_tls12_split_key_block_cbc(cipher, mac, keyblk, need, out);
    wipe(keyblk, sizeof(keyblk));
    return r;
}

extern "C" int tlsrec_tls12_export_keying_material(int prf, const unsigned char master[48],
                                                   const unsigned char randbytes[64], const char *label,
                                                   size_t label_len, const unsigned char *context,
                                                   size_t context_len, int use_context, unsigned char *out,
                                                   size_t out_len)
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (use_context && context_len > 65535) return TLSREC_ERR_SSL_BAD_INPUT_DATA;     /* ssl_tls.c:8905 */
    if (out_len == 0) return 0;
    if (!master || !randbytes || (use_context && context_len && !context)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* client_random || server_random [|| uint16 context_len || context], ssl_tls.c:8920-8929 */
    unsigned char head[66];
    memcpy(head, randbytes + 32, 32);
    memcpy(head + 32, randbytes, 32);
    head[64] = (unsigned char) (context_len >> 8);
    head[65] = (unsigned char) context_len;
    return prf_run(a, master, 48, label, label_len, head, use_context ? 66 : 64, context,
                   use_context ? context_len : 0, out, out_len);
}

template <int ALG, int KL, int IVL> static hipError_t tls12_launch(const Tls12Args &a, hipStream_t st)
{
    hipLaunchKernelGGL((tls12_derive_kernel<ALG, KL, IVL>), dim3((a.count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

static int tls12_check(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int prf,
                       const tlsrec_tls12_conn *conns)
{
    if (!kt || (!conns && count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const uint32_t cap = tlsrec_keytab_capacity(kt);
    if (first > cap || (uint64_t) count * 2 > (uint64_t) (cap - first)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (tlsrec_cipher_keylen(cipher) == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (prf_index(prf) < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    return 0;
}

/* The derive kernel alone (see tlsrec__tls13_stage_keys). */
extern "C" int tlsrec__tls12_stage_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int prf,
                                        const tlsrec_tls12_conn *conns, void *stream)
{
    int r = tls12_check(kt, first, count, cipher, prf, conns);
    if (r != 0 || count == 0) return r;
    const int alg = prf_index(prf);
    const uint32_t kl = tlsrec_cipher_keylen(cipher);
    Tls12Args a;
    a.conns = conns;
    a.out = tlsrec__keytab_stage(kt) + first;
    a.count = count;
    a.cipher = (uint32_t) cipher;
    a.taglen = tlsrec_cipher_taglen(cipher);
    a.aligned = ((uintptr_t) conns & 15) == 0;     /* 112-byte records: 16-byte loads if the array is aligned */
    hipStream_t st = (hipStream_t) stream;
    hipError_t e;
    if (alg == H_SHA384) {
        e = cipher == TLSREC_CIPHER_CHACHA20_POLY1305 ? tls12_launch<H_SHA384, 32, 12>(a, st)
            : kl == 16 ? tls12_launch<H_SHA384, 16, 4>(a, st)
            : kl == 24 ? tls12_launch<H_SHA384, 24, 4>(a, st) : tls12_launch<H_SHA384, 32, 4>(a, st);
    } else {
        e = cipher == TLSREC_CIPHER_CHACHA20_POLY1305 ? tls12_launch<H_SHA256, 32, 12>(a, st)
            : kl == 16 ? tls12_launch<H_SHA256, 16, 4>(a, st)
            : kl == 24 ? tls12_launch<H_SHA256, 24, 4>(a, st) : tls12_launch<H_SHA256, 32, 4>(a, st);
    }
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls12_keytab_derive(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int prf,
                                          const tlsrec_tls12_conn *conns, void *stream)
{
    int r = tlsrec__tls12_stage_keys(kt, first, count, cipher, prf, conns, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, 2 * count, cipher, (hipStream_t) stream);
    return r;
}

/* ---- the same for the CBC + HMAC suites ---- */
extern "C" tlsrec_cbc_key_material *tlsrec__keytab_stage_cbc(tlsrec_keytab *kt);
extern "C" int tlsrec__keytab_commit_staged_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int mac,
                                                int etm, hipStream_t st);

template <int ALG, int KL, int ML> static hipError_t tls12_launch_cbc(const Tls12CbcArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL((tls12_derive_cbc_kernel<ALG, KL, ML>), dim3((a.count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <int ALG, int KL> static hipError_t tls12_launch_cbc_mac(size_t ml, const Tls12CbcArgs &a, hipStream_t st)
{
    return ml == 20 ? tls12_launch_cbc<ALG, KL, 20>(a, st)
           : ml == 32 ? tls12_launch_cbc<ALG, KL, 32>(a, st) : tls12_launch_cbc<ALG, KL, 48>(a, st);
}

/* The derive kernel alone: 2 * count tlsrec_cbc_key_material records into the
 * table's CBC staging area, nothing committed (see tlsrec__tls13_stage_keys). */
extern "C" int tlsrec__tls12_stage_keys_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int mac,
                                            int etm, int prf, const tlsrec_tls12_conn *conns, void *stream)
{
    if (!kt || (!conns && count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const uint32_t cap = tlsrec_keytab_capacity(kt);
    if (first > cap || (uint64_t) count * 2 > (uint64_t) (cap - first)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t kl = cbc_split_keylen(cipher), ml = cbc_split_maclen(mac);
    if (!cbc_split_pair_ok(cipher, mac)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    const int alg = prf_index(prf);
    if (alg < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (etm < 0 || etm > 1) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    tlsrec_cbc_key_material *stage = tlsrec__keytab_stage_cbc(kt);
    if (!stage) return TLSREC_ERR_SSL_ALLOC_FAILED;
    Tls12CbcArgs a;
    a.conns = conns;
    a.out = stage + first;
    a.count = count;
    a.head = (uint32_t) cipher | (3u << 8) | ((uint32_t) mac << 16) | ((uint32_t) etm << 24);
    a.aligned = ((uintptr_t) conns & 15) == 0;
    hipStream_t st = (hipStream_t) stream;
    hipError_t e;
    if (alg == H_SHA384)
        e = kl == 16 ? tls12_launch_cbc_mac<H_SHA384, 16>(ml, a, st) : tls12_launch_cbc_mac<H_SHA384, 32>(ml, a, st);
    else
        e = kl == 16 ? tls12_launch_cbc_mac<H_SHA256, 16>(ml, a, st) : tls12_launch_cbc_mac<H_SHA256, 32>(ml, a, st);
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls12_keytab_derive_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int mac,
                                              int etm, int prf, const tlsrec_tls12_conn *conns, void *stream)
{
    int r = tlsrec__tls12_stage_keys_cbc(kt, first, count, cipher, mac, etm, prf, conns, stream);
    if (r == 0 && count)
        r = tlsrec__keytab_commit_staged_cbc(kt, first, 2 * count, cipher, mac, etm, (hipStream_t) stream);
    return r;
}

/* ---- the handshake before the key expansion: master secret, Finished ---- */
extern "C" int tlsrec_tls12_calc_finished(int prf, const unsigned char master[48], const unsigned char *transcript_hash,
                                          int from, unsigned char out[12])
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (from != TLSREC_IS_CLIENT && from != TLSREC_IS_SERVER) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!master || !transcript_hash || !out) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* ssl_tls.c:7217-7219, :7252 */
    const char *lbl = from == TLSREC_IS_CLIENT ? "client finished" : "server finished";
    return prf_run(a, master, 48, lbl, 15, transcript_hash, alg_len(a), nullptr, 0, out, 12);
}

template <class T, bool EMS> static hipError_t tls12_launch_master(const Tls12MasterArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL((tls12_master_kernel<T, EMS>), dim3((a.count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

extern "C" int tlsrec_tls12_batch_compute_master(int prf, uint32_t pms_len, int extended_ms,
                                                 const tlsrec_tls12_pms_conn *conns, tlsrec_tls12_conn *out,
                                                 uint32_t count, void *stream)
{
    const int alg = prf_index(prf);
    if (alg < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if ((!conns || !out) && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (pms_len == 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (pms_len > sizeof(conns->premaster)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (count == 0) return 0;
    static const int device = tlsrec_device_check();     /* no key table vouches for a device here; asked once */
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls12MasterArgs a;
    a.conns = conns;
    a.out = out;
    a.count = count;
    a.pms_len = pms_len;
    a.aligned = al(conns, AL_CONNS) | al(out, AL_AUX);     /* 240- and 112-byte records */
    hipStream_t st = (hipStream_t) stream;
    hipError_t e;
    if (alg == H_SHA384) e = extended_ms ? tls12_launch_master<L384, true>(a, st) : tls12_launch_master<L384, false>(a, st);
    else e = extended_ms ? tls12_launch_master<L256, true>(a, st) : tls12_launch_master<L256, false>(a, st);
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls12_batch_verify_data(int prf, int from, const tlsrec_tls12_conn *conns,
                                              const tlsrec_tls13_secret *transcripts, const uint8_t *offered,
                                              uint8_t *verify, uint32_t *match, uint32_t count, void *stream)
{
    const int alg = prf_index(prf);
    if (alg < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (from != TLSREC_IS_CLIENT && from != TLSREC_IS_SERVER) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if ((!conns || !transcripts) && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if ((offered == nullptr) != (match == nullptr)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!verify && !match && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    static const int device = tlsrec_device_check();
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls12FinishedArgs a;
    a.conns = conns;
    a.transcripts = transcripts;
    a.offered = offered;
    a.verify = verify;
    a.match = match;
    a.count = count;
    a.aligned = al(conns, AL_CONNS) | al(transcripts, AL_TRANSCRIPT) | al(offered, AL_OFFERED12) | al(verify, AL_VERIFY);
    /* "client finished" / "server finished" (ssl_tls.c:7217-7219): the first two cells differ */
    a.l0 = from == TLSREC_IS_CLIENT ? 0x636c6965u : 0x73657276u;
    a.l1 = from == TLSREC_IS_CLIENT ? 0x6e742066u : 0x65722066u;
    hipStream_t st = (hipStream_t) stream;
    if (alg == H_SHA384) hipLaunchKernelGGL(tls12_finished_kernel<L384>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(tls12_finished_kernel<L256>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls12_batch_export_keying_material(int prf, const tlsrec_tls12_conn *conns, const char *label,
                                                         size_t label_len, const uint8_t *contexts,
                                                         uint32_t context_len, uint32_t context_stride,
                                                         int use_context, uint8_t *out, uint32_t out_len,
                                                         uint32_t out_stride, uint32_t count, void *stream)
{
    const int alg = prf_index(prf);
    if (alg < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const int r = export_check(conns, contexts, out, label, label_len, use_context != 0, context_len, context_stride,
                               out_len, out_stride, count);
    if (r != 0 || count == 0 || out_len == 0) return r;
    static const int device = tlsrec_device_check();
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls12ExportArgs a;
    memset(&a, 0, sizeof(a));
    a.conns = conns;
    a.contexts = contexts;
    a.out = out;
    a.count = count;
    a.label_len = (uint32_t) label_len;
    a.use_context = use_context != 0;
    a.context_len = use_context ? context_len : 0;
    a.context_stride = use_context ? context_stride : 0;
    a.out_len = out_len;
    a.out_stride = out_stride;
    a.aligned = al(conns, AL_CONNS) | al_out(out, out_stride);
    for (size_t k = 0; k < label_len; k++) a.label[k >> 2] |= (uint32_t) (unsigned char) label[k] << (24 - 8 * (k & 3));
    hipStream_t st = (hipStream_t) stream;
    if (alg == H_SHA384) hipLaunchKernelGGL(tls12_export_kernel<L384>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(tls12_export_kernel<L256>, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

/* ---- DTLS cookies (library/ssl_cookie.c; ssl_msg.c:3322-3454) ---- */
struct tlsrec_cookie_ctx {
    uint32_t *mid;          /* device: ip[8], op[8], then the 32 bytes the key is staged in */
    uint32_t timeout;       /* ctx->timeout */
};

extern "C" int tlsrec_cookie_setup(tlsrec_cookie_ctx **ctx, const unsigned char key[32], uint32_t timeout)
{
    if (!ctx) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    *ctx = nullptr;
    if (tlsrec_device_check() != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    unsigned char k[32];
    if (key) {
        memcpy(k, key, 32);
    } else {
        /* psa_generate_key (ssl_cookie.c:105) */
        for (size_t got = 0; got < sizeof(k);) {
            const ssize_t r = getrandom(k + got, sizeof(k) - got, 0);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) {
                wipe(k, sizeof(k));
                return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
            }
            got += (size_t) r;
        }
    }
    tlsrec_cookie_ctx *c = (tlsrec_cookie_ctx *) calloc(1, sizeof(*c));
    int r = c ? 0 : TLSREC_ERR_SSL_ALLOC_FAILED;
    if (r == 0 && hipMalloc((void **) &c->mid, 64 + 32) != hipSuccess) {
        c->mid = nullptr;
        r = TLSREC_ERR_SSL_ALLOC_FAILED;
    }
    if (r == 0) {
        uint8_t *dkey = (uint8_t *) (c->mid + 16);
        hipError_t e = hipMemcpy(dkey, k, 32, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(cookie_setup_kernel, dim3(1), dim3(64), 0, (hipStream_t) nullptr, c->mid, dkey);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    wipe(k, sizeof(k));
    if (r != 0) {
        tlsrec_cookie_free(c);
        return r;
    }
    c->timeout = timeout;
    *ctx = c;
    return 0;
}

extern "C" void tlsrec_cookie_set_timeout(tlsrec_cookie_ctx *ctx, uint32_t delay)
{
    if (ctx) ctx->timeout = delay;
}

extern "C" void tlsrec_cookie_free(tlsrec_cookie_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->mid) {
        hipMemset(ctx->mid, 0, 64 + 32);
        hipDeviceSynchronize();
        hipFree(ctx->mid);
    }
    wipe(ctx, sizeof(*ctx));
    free(ctx);
}

static int cookie_launch(int mode, const tlsrec_cookie_ctx *ctx, uint64_t now, const void *items, uint32_t n,
                         const uint8_t *arena, const uint8_t *id_arena, uint8_t *out, int32_t *status, bool prefill,
                         hipStream_t st)
{
    CookieArgs a;
    a.mid = ctx->mid;
    a.items = items;
    a.arena = arena;
    a.id_arena = id_arena;
    a.out = out;
    a.status = status;
    a.now = now;
    a.timeout = ctx->timeout;
    a.n = n;
    const dim3 grid((n + 63) / 64), block(64);
    if (prefill)
        hipLaunchKernelGGL(cookie_prefill_kernel, grid, block, 0, st, status, n, mode == CK_HELLO ? 2u : 1u);
    if (mode == CK_WRITE) hipLaunchKernelGGL(cookie_kernel<CK_WRITE>, grid, block, 0, st, a);
    else if (mode == CK_CHECK) hipLaunchKernelGGL(cookie_kernel<CK_CHECK>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(cookie_kernel<CK_HELLO>, grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_cookie_batch_write(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_cookie_item *items,
                                         uint32_t n, const uint8_t *id_arena, uint8_t *cookie_arena, int32_t *status,
                                         void *stream)
{
    if (!ctx || (n && (!items || !id_arena || !cookie_arena || !status))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (n == 0) return 0;
    return cookie_launch(CK_WRITE, ctx, now, items, n, nullptr, id_arena, cookie_arena, status, true,
                         (hipStream_t) stream);
}

extern "C" int tlsrec_cookie_batch_check(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_cookie_item *items,
                                         uint32_t n, const uint8_t *id_arena, const uint8_t *cookie_arena,
                                         int32_t *status, void *stream)
{
    if (!ctx || (n && (!items || !id_arena || !cookie_arena || !status))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (n == 0) return 0;
    return cookie_launch(CK_CHECK, ctx, now, items, n, cookie_arena, id_arena, nullptr, status, true,
                         (hipStream_t) stream);
}

extern "C" int tlsrec_dtls_check_clihlo_cookies(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_clihlo *hellos,
                                                uint32_t n, const uint8_t *arena, const uint8_t *id_arena,
                                                uint8_t *out_arena, tlsrec_clihlo_res *res, void *stream)
{
    if (!ctx || (n && (!hellos || !arena || !id_arena || !out_arena || !res))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (n == 0) return 0;
    return cookie_launch(CK_HELLO, ctx, now, hellos, n, arena, id_arena, out_arena, &res->status, true,
                         (hipStream_t) stream);
}

/* One client in host buffers: a batch of one staged in the single-shot arena
 * (item at 0, status at 32, cookie at 64, id at 96). */
static int cookie_single(int mode, tlsrec_cookie_ctx *ctx, unsigned char *cookie, size_t cookie_len,
                         const unsigned char *cli_id, size_t cli_id_len)
{
    enum { AT_STATUS = 32, AT_COOKIE = 64, AT_ID = 96, BYTES = 96 + 256 };
    uint8_t h[BYTES];
    memset(h, 0, sizeof(h));
    tlsrec_cookie_item it;
    it.id_off = AT_ID;
    it.cookie_off = AT_COOKIE;
    it.id_len = cli_id_len > 255 ? 256u : (uint32_t) cli_id_len;
    it.cookie_len = cookie_len > 0xffffffffu ? 0xffffffffu : (uint32_t) cookie_len;
    memcpy(h, &it, sizeof(it));
    const int32_t unreached = TLSREC_ERR_SSL_INTERNAL_ERROR;
    memcpy(h + AT_STATUS, &unreached, 4);
    if (mode == CK_CHECK && cookie_len == TLSREC_COOKIE_LEN) memcpy(h + AT_COOKIE, cookie, TLSREC_COOKIE_LEN);
    if (it.id_len <= 255) memcpy(h + AT_ID, cli_id, it.id_len);
    const uint64_t now = (uint64_t) time(nullptr);
    pthread_mutex_lock(&g_ks_mu);
    int r = ks_init_locked();
    if (r == 0) {
        hipError_t e = hipMemcpyAsync(g_ks_dev, h, BYTES, hipMemcpyHostToDevice, g_ks_stream);
        if (e == hipSuccess &&
            cookie_launch(mode, ctx, now, g_ks_dev, 1, g_ks_dev, g_ks_dev, g_ks_dev, (int32_t *) (g_ks_dev + AT_STATUS),
                          false, g_ks_stream) != 0)
            e = hipErrorLaunchFailure;
        if (e == hipSuccess)
            e = hipMemcpyAsync(h + AT_STATUS, g_ks_dev + AT_STATUS, AT_ID - AT_STATUS, hipMemcpyDeviceToHost, g_ks_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_ks_stream);
        if (e != hipSuccess) r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    pthread_mutex_unlock(&g_ks_mu);
    if (r == 0) {
        int32_t st;
        memcpy(&st, h + AT_STATUS, 4);
        r = st;
        if (mode == CK_WRITE && st == 0) memcpy(cookie, h + AT_COOKIE, TLSREC_COOKIE_LEN);
    }
    return r;
}

extern "C" int tlsrec_cookie_write(void *ctx, unsigned char **p, unsigned char *end, const unsigned char *cli_id,
                                   size_t cli_id_len)
{
    if (!ctx || !cli_id || !p || !*p) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t space = end > *p ? (size_t) (end - *p) : 0;
    const int r = cookie_single(CK_WRITE, (tlsrec_cookie_ctx *) ctx, *p, space, cli_id, cli_id_len);
    if (r == 0) *p += TLSREC_COOKIE_LEN;
    return r;
}

extern "C" int tlsrec_cookie_check(void *ctx, const unsigned char *cookie, size_t cookie_len, const unsigned char *cli_id,
                                   size_t cli_id_len)
{
    if (!ctx || !cli_id || (!cookie && cookie_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return cookie_single(CK_CHECK, (tlsrec_cookie_ctx *) ctx, (unsigned char *) cookie, cookie_len, cli_id, cli_id_len);
}
