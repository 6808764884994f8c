/*
 * tlsrec_kdf.h -- the word-wise HMAC / HKDF / P_hash building blocks of the
 * one-lane-per-connection key-derivation kernels (tls13_ladder.hip,
 * tls12_batch.hip, exporter.hip, cookie.hip) on the compression of
 * tlsrec_sha.h, and the small host-side helpers those units and keysched.hip
 * share.
 *
 * Device side: every message is put together in registers as big-endian
 * 32-bit cells, 16 to a SHA-256 block and 32 to a SHA-512 one, with its
 * padding and length word in place; the two HMAC midstates of a key (key ^
 * ipad, key ^ opad) are computed once and serve every HMAC under it.  All
 * functions are __forceinline__: nothing is shared through the linker.
 */
#ifndef TLSREC_KDF_H
#define TLSREC_KDF_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_internal.h"
#include "tlsrec_sha.h"

namespace tlsks {

enum { H_SHA256 = 0, H_SHA384 = 1 };

/* a big-endian 32-bit word of device memory, by one aligned load or by bytes */
__device__ __forceinline__ uint32_t load_be32(const uint8_t *p, bool aligned)
{
    if (aligned) return __builtin_bswap32(*reinterpret_cast<const uint32_t *>(p));
    return ((uint32_t) p[0] << 24) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 8) | p[3];
}

/* The per-hash traits of the blocks below: the compression S of tlsrec_sha.h with its word W, the digest in words
 * (HW), cells (HC) and bytes (HB), the block (BB) and its length field (LENB) in bytes. */
struct L256 {
    typedef S256 S;
    typedef uint32_t W;
    enum { HW = 8, HC = 8, HB = 32, BB = 64, LENB = 8 };
    static __device__ __forceinline__ W iv(int j) { return S::iv(j); }
};
struct L384 {
    typedef S512 S;
    typedef uint64_t W;
    enum { HW = 6, HC = 12, HB = 48, BB = 128, LENB = 16 };
    static __device__ __forceinline__ W iv(int j) { return S::iv(j); }
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

/* ... under an H-byte key */
template <class T>
__device__ __forceinline__ void hmac_mid(const typename T::W (&key)[T::HW], typename T::W (&ip)[8], typename T::W (&op)[8])
{
    typename T::W kb[16];
#pragma unroll
    for (int j = 0; j < 16; j++) kb[j] = j < T::HW ? key[j] : (typename T::W) 0;
    hmac_mid_block<T>(kb, ip, op);
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

/* block `blk` of a message of n bytes held in the cells m[] (n wave-uniform; blk
 * a constant at every call, so every index is one; the caller asks for the
 * blocks up to the one that ends the padded message and no further): bytes past
 * n are masked off, 0x80 follows the message and the length closes the last
 * block.  PRE: the bytes hashed before the message, which the length counts --
 * the key block of an HMAC, 0 for a plain hash; NO_PAD: neither 0x80 nor a
 * length, the zero-padded block of an HMAC key. */
enum { NO_PAD = -1 };
template <class T, int NC, int PRE = (int) T::BB>
__device__ __forceinline__ void msg_block(typename T::W (&w)[16], const uint32_t (&m)[NC], uint32_t n, int blk)
{
    constexpr int CPB = T::BB / 4;
    constexpr bool PAD = PRE != NO_PAD;
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
    if (PAD && (int) n + 1 + (int) T::LENB <= (blk + 1) * (int) T::BB) w[15] = (typename T::W) ((PRE + n) * 8);
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

enum { AL_CONNS = 1, AL_TRAFFIC = 2, AL_AUX = 4, AL_MASTER = 8, AL_TRANSCRIPT = 16 };

/* The 77-byte TLS 1.2 PRF seed of a 13-byte label and the 64 random bytes R as
 * cells: l0..l2 are the label's first 12 characters, l3 its last one in the top
 * byte.  The label leaves the random words one byte off; S[19] holds the last
 * byte alone (msg_block places the 0x80). */
__device__ __forceinline__ void tls12_seed77(uint32_t (&S)[20], uint32_t l0, uint32_t l1, uint32_t l2, uint32_t l3,
                                             const uint32_t (&R)[16])
{
    S[0] = l0;
    S[1] = l1;
    S[2] = l2;
    S[3] = l3 | (R[0] >> 8);
#pragma unroll
    for (int k = 1; k < 16; k++) S[3 + k] = (R[k - 1] << 24) | (R[k] >> 8);
    S[19] = R[15] << 24;
}

/* ---------------- host side --------------------------------------------- */
static const size_t MAX_LABEL = 249;        /* MBEDTLS_SSL_TLS1_3_HKDF_LABEL_MAX_LABEL_LEN, ssl_tls13_keys.h:66 */

static inline int alg_index(int hash_alg)
{
    return hash_alg == TLSREC_ALG_SHA_256 ? H_SHA256 : hash_alg == TLSREC_ALG_SHA_384 ? H_SHA384 : -1;
}

static inline int prf_index(int prf)
{
    return prf == TLSREC_TLS_PRF_SHA256 ? H_SHA256 : prf == TLSREC_TLS_PRF_SHA384 ? H_SHA384 : -1;
}

static inline size_t alg_len(int idx) { return idx == H_SHA384 ? 48 : 32; }

/* f(L384()) or f(L256()) for alg = H_SHA384 / H_SHA256: one call site for the two instantiations of a launch */
template <class F> static inline auto by_hash(int alg, F f) { return alg == H_SHA384 ? f(L384()) : f(L256()); }

/* one lane per item, 64 to a workgroup */
template <class K, class A> static inline hipError_t launch_lanes(K kernel, uint32_t count, hipStream_t st, const A &a)
{
    hipLaunchKernelGGL(kernel, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

static inline int launch_status(hipError_t e) { return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED; }

/* For the batch calls that take no key table, which would vouch for a device: asked once per process. */
TLSREC_LOCAL inline bool device_ready()
{
    static const int device = tlsrec_device_check();
    return device == 0;
}

/* `slots` key-table slots from `first` on lie inside the table */
static inline bool keytab_range_ok(const tlsrec_keytab *kt, uint32_t first, uint64_t slots)
{
    const uint32_t cap = tlsrec_keytab_capacity(kt);
    return first <= cap && slots <= (uint64_t) (cap - first);
}

/* ssl_tls13_hkdf_encode_label, ssl_tls13_keys.c:98-136 (without the context
 * bytes when ctx == NULL: the caller appends a device-computed context) */
static inline size_t encode_label(size_t desired, const unsigned char *label, size_t label_len,
                                  const unsigned char *ctx, size_t ctx_len, uint8_t *dst)
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

/* HkdfLabel(desired, label, context of ctx_len bytes to follow) as the kernels' cells */
static inline LabelW label_cells(size_t desired, const void *label, size_t label_len, size_t ctx_len)
{
    uint8_t b[24] = { 0 };
    encode_label(desired, (const unsigned char *) label, label_len, nullptr, ctx_len, b);
    LabelW l;
    for (int c = 0; c < 6; c++)
        l.c[c] = ((uint32_t) b[4 * c] << 24) | ((uint32_t) b[4 * c + 1] << 16) | ((uint32_t) b[4 * c + 2] << 8) | b[4 * c + 3];
    return l;
}

/* the AL_* bit of an array the kernels may address with 16-byte loads and stores */
static inline uint32_t al(const void *p, uint32_t bit) { return ((uintptr_t) p & 15) == 0 ? bit : 0u; }

/* ... of an output array with a stride (AL_AUX): 16-byte stores need the base and the stride aligned */
static inline uint32_t al_out(const void *out, uint32_t stride) { return (stride & 15) == 0 ? al(out, AL_AUX) : 0u; }

static inline void wipe(void *p, size_t n)
{
    volatile uint8_t *v = (volatile uint8_t *) p;
    for (size_t i = 0; i < n; i++) v[i] = 0;
}

/* The shapes of a TLS 1.2 key block, for the single-shot calls (keysched.hip) and the batches (tls12_batch.hip). */
/* fixed_ivlen of a TLS 1.2 AEAD transform, ssl_tls.c:7722-7727 */
static inline size_t tls12_fixed_ivlen(int cipher) { return cipher == TLSREC_CIPHER_CHACHA20_POLY1305 ? 12 : 4; }

/* the CBC + HMAC suites' layout (mac_key_len != 0), ssl_tls.c:7858-7886:
 * client_mac | server_mac | client_key | server_key (TLS 1.2 carries the CBC
 * IV in each record, so the IV part of the block goes unused) */
static inline size_t cbc_split_keylen(int cipher)
{
    switch (cipher) {
        case TLSREC_CIPHER_AES_128_CBC: case TLSREC_CIPHER_ARIA_128_CBC: case TLSREC_CIPHER_CAMELLIA_128_CBC: return 16;
        case TLSREC_CIPHER_AES_256_CBC: case TLSREC_CIPHER_ARIA_256_CBC: case TLSREC_CIPHER_CAMELLIA_256_CBC: return 32;
        default: return 0;
    }
}
static inline size_t cbc_split_maclen(int mac)
{
    return mac == TLSREC_MAC_SHA1 ? 20 : mac == TLSREC_MAC_SHA256 ? 32 : mac == TLSREC_MAC_SHA384 ? 48 : 0;
}
/* a pair tlsrec_keytab_load_cbc takes: AES with every MAC, an ARIA / Camellia id
 * only with its suites' MAC (128-bit keys SHA-256, 256-bit keys SHA-384) */
static inline bool cbc_split_pair_ok(int cipher, int mac)
{
    const size_t kl = cbc_split_keylen(cipher), ml = cbc_split_maclen(mac);
    if (kl == 0 || ml == 0) return false;
    if (cipher <= TLSREC_CIPHER_AES_256_CBC) return true;
    return mac == (kl == 16 ? TLSREC_MAC_SHA256 : TLSREC_MAC_SHA384);
}

/* tls13_ladder.hip: the constants of LadderConsts for each hash */
template <class T> const LadderConsts<T> &ladder_consts();
template <> TLSREC_LOCAL const LadderConsts<L256> &ladder_consts<L256>();
template <> TLSREC_LOCAL const LadderConsts<L384> &ladder_consts<L384>();

} /* namespace tlsks */

#endif /* TLSREC_KDF_H */

