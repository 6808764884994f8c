/*
 * tlsrec_cbc.h -- building blocks of the AES-CBC + HMAC record path (cbc.hip):
 * the MAC_THEN_ENCRYPT / ENCRYPT_THEN_MAC branches of mbedtls_ssl_encrypt_buf /
 * mbedtls_ssl_decrypt_buf (ssl_msg.c:906-968, :1080-1253, :1435-1702,
 * :1717-1801).
 *
 *   - SHA-1 / SHA-256 / SHA-512 compression on whole words held in registers,
 *     each started from a stored midstate (the hash state after the HMAC
 *     ipad / opad block, made once per key by the key setup);
 *   - HMAC over "additional data || record bytes" as one loop with a single
 *     compression call site, whose trip count and memory accesses depend only
 *     on public lengths (cbc_hmac, the mbedtls_ct_hmac of ssl_msg.c:1757);
 *   - the AES equivalent inverse cipher on LDS tables laid out like the
 *     encryption tables (a copy per bank: conflict-free for any index);
 *   - the key schedule of both directions.
 *
 * Everything is __host__ __device__ and free of device builtins on the host
 * side, so a CPU build can check it against a reference implementation.
 */
#ifndef TLSREC_CBC_H
#define TLSREC_CBC_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "tlsrec.h"

namespace tlsrec {

#define TLSREC_CBC_HD __host__ __device__ __forceinline__

TLSREC_CBC_HD uint32_t cbc_maclen(int mac)
{
    return mac == TLSREC_MAC_SHA1 ? 20u : mac == TLSREC_MAC_SHA256 ? 32u : mac == TLSREC_MAC_SHA384 ? 48u : 0u;
}
TLSREC_CBC_HD uint32_t cbc_keylen(int cipher)
{
    return (cipher == TLSREC_CIPHER_AES_128_CBC || cipher == TLSREC_CIPHER_ARIA_128_CBC ||
            cipher == TLSREC_CIPHER_CAMELLIA_128_CBC) ? 16u
           : (cipher == TLSREC_CIPHER_AES_256_CBC || cipher == TLSREC_CIPHER_ARIA_256_CBC ||
              cipher == TLSREC_CIPHER_CAMELLIA_256_CBC) ? 32u : 0u;
}
/* (id 25 lies inside [CBC_FIRST, CBC_LAST] and is no cipher) */
TLSREC_CBC_HD int cbc_is_cipher(int c)
{
    return c >= TLSREC_CIPHER_CBC_FIRST && c <= TLSREC_CIPHER_CBC_LAST && c != TLSREC_CIPHER_AES_256_CBC + 1;
}
/* AES-CBC alone: the key length, 0 for every other id (the AES record kernels' slot filter) */
TLSREC_CBC_HD uint32_t cbc_aes_keylen(int cipher)
{
    return cipher == TLSREC_CIPHER_AES_128_CBC ? 16u : cipher == TLSREC_CIPHER_AES_256_CBC ? 32u : 0u;
}
/* ARIA-CBC / Camellia-CBC: the S-box image ciphers (cbc_alt.hip) */
TLSREC_CBC_HD int cbc_is_alt(int c) { return c >= TLSREC_CIPHER_ARIA_128_CBC && c <= TLSREC_CIPHER_CAMELLIA_256_CBC; }
/* the round count that picks a slot's record kernel: AES 10 / 14, ARIA 12 / 16
 * (RFC 5794 2.1), Camellia 18 / 24 (RFC 3713 2.3); 0 for no CBC cipher */
TLSREC_CBC_HD uint32_t cbc_nr(int c)
{
    const uint32_t kl = cbc_keylen(c);
    if (kl == 0) return 0u;
    if (c >= TLSREC_CIPHER_CAMELLIA_128_CBC) return kl == 16 ? 18u : 24u;
    return kl / 4 + (c >= TLSREC_CIPHER_ARIA_128_CBC ? 8u : 6u);
}
/* The (cipher, MAC) pairs a slot can hold: AES-CBC with every MAC; ARIA and
 * Camellia only as the reference's suites pair them (ssl_ciphersuites.c:
 * 128-bit keys with SHA-256, 256-bit keys with SHA-384). */
TLSREC_CBC_HD int cbc_pair_ok(int cipher, int mac)
{
    if (cbc_keylen(cipher) == 0 || cbc_maclen(mac) == 0) return 0;
    if (!cbc_is_alt(cipher)) return 1;
    return mac == (cbc_keylen(cipher) == 16 ? TLSREC_MAC_SHA256 : TLSREC_MAC_SHA384);
}
/* bit of a (cipher, MAC) pair in the key table's variants word (tlsrec__launch_cbc) */
TLSREC_CBC_HD uint32_t cbc_variant_bit(int cipher, int mac)
{
    return 1u << (3 * (cipher - TLSREC_CIPHER_CBC_FIRST) + (mac - 1));
}

/* Per-slot CBC state beyond SlotState (AES: rk / rkr encryption round keys,
 * ark decryption round keys; ARIA / Camellia the other way round: ark the
 * encryption keys as in their GCM slots, the decryption key array at the start
 * of rk / rkr; km.reserved[1] = mac, [2] = etm): the HMAC midstates
 * as 32-bit words at the start of the slot's GHASH table area, which a CBC
 * slot does not otherwise use -- inner at words 0..15, outer at 16..31
 * (SHA-512 words as high, low pairs). */
constexpr int CBC_MS_OUTER = 16;
constexpr int CBC_MS_WORDS = 32;

/* ---------------- hashes ------------------------------------------------ */
template <int MAC> struct CbcHash;
template <> struct CbcHash<TLSREC_MAC_SHA1> { static constexpr int B = 64, LENB = 8, NS = 5, DIGW = 5; };
template <> struct CbcHash<TLSREC_MAC_SHA256> { static constexpr int B = 64, LENB = 8, NS = 8, DIGW = 8; };
/* SHA-384: the SHA-512 compression, 16 state words (high, low), 12 of digest */
template <> struct CbcHash<TLSREC_MAC_SHA384> { static constexpr int B = 128, LENB = 16, NS = 16, DIGW = 12; };
template <int MAC> struct CbcTag {};

TLSREC_CBC_HD uint32_t cbc_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
TLSREC_CBC_HD uint32_t cbc_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
TLSREC_CBC_HD uint64_t cbc_rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
TLSREC_CBC_HD uint32_t cbc_bswap(uint32_t x) { return __builtin_bswap32(x); }

TLSREC_CBC_HD void cbc_hash_iv(CbcTag<TLSREC_MAC_SHA1>, uint32_t (&st)[5])
{
    st[0] = 0x67452301u; st[1] = 0xefcdab89u; st[2] = 0x98badcfeu; st[3] = 0x10325476u; st[4] = 0xc3d2e1f0u;
}
TLSREC_CBC_HD void cbc_hash_iv(CbcTag<TLSREC_MAC_SHA256>, uint32_t (&st)[8])
{
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}
TLSREC_CBC_HD void cbc_hash_iv(CbcTag<TLSREC_MAC_SHA384>, uint32_t (&st)[16])
{
    st[0] = 0xcbbb9d5du; st[1] = 0xc1059ed8u; st[2] = 0x629a292au; st[3] = 0x367cd507u;
    st[4] = 0x9159015au; st[5] = 0x3070dd17u; st[6] = 0x152fecd8u; st[7] = 0xf70e5939u;
    st[8] = 0x67332667u; st[9] = 0xffc00b31u; st[10] = 0x8eb44a87u; st[11] = 0x68581511u;
    st[12] = 0xdb0c2e0du; st[13] = 0x64f98fa7u; st[14] = 0x47b5481du; st[15] = 0xbefa4fa4u;
}

/* SHA-1 (FIPS 180-4 6.1.2), the schedule as a 16-word ring */
TLSREC_CBC_HD void cbc_compress(CbcTag<TLSREC_MAC_SHA1>, uint32_t (&st)[5], const uint32_t (&m)[16])
{
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = m[i];
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
#pragma unroll
    for (int t = 0; t < 80; t++) {
        if (t >= 16) w[t & 15] = cbc_rotl(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1);
        uint32_t f, k;
        if (t < 20) { f = (b & c) | (~b & d); k = 0x5a827999u; }
        else if (t < 40) { f = b ^ c ^ d; k = 0x6ed9eba1u; }
        else if (t < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8f1bbcdcu; }
        else { f = b ^ c ^ d; k = 0xca62c1d6u; }
        const uint32_t tmp = cbc_rotl(a, 5) + f + e + k + w[t & 15];
        e = d; d = c; c = cbc_rotl(b, 30); b = a; a = tmp;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e;
}

/* SHA-256 (FIPS 180-4 6.2.2): 16 rounds on the block, then three times 16
 * rounds that extend the ring in place */
TLSREC_CBC_HD void cbc_compress(CbcTag<TLSREC_MAC_SHA256>, uint32_t (&st)[8], const uint32_t (&m)[16])
{
    static constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u
    };
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = m[i];
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#define TLSREC_CBC_R256(ki)                                                                             \
    {                                                                                                   \
        const uint32_t t1 = h + (cbc_rotr(e, 6) ^ cbc_rotr(e, 11) ^ cbc_rotr(e, 25)) + ((e & f) ^ (~e & g)) + \
                            (ki) + w[i];                                                                \
        const uint32_t t2 = (cbc_rotr(a, 2) ^ cbc_rotr(a, 13) ^ cbc_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c)); \
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;                              \
    }
#pragma unroll
    for (int i = 0; i < 16; i++) TLSREC_CBC_R256(K[i])
#pragma unroll 1
    for (int r = 16; r < 64; r += 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
            w[i] += (cbc_rotr(y, 17) ^ cbc_rotr(y, 19) ^ (y >> 10)) + w[(i + 9) & 15] +
                    (cbc_rotr(x, 7) ^ cbc_rotr(x, 18) ^ (x >> 3));
            TLSREC_CBC_R256(K[r + i])
        }
    }
#undef TLSREC_CBC_R256
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

/* SHA-512 (FIPS 180-4 6.4.2) for SHA-384; m holds the block as 32 big-endian
 * 32-bit words, st the state as (high, low) pairs */
TLSREC_CBC_HD void cbc_compress(CbcTag<TLSREC_MAC_SHA384>, uint32_t (&st)[16], const uint32_t (&m)[32])
{
    static constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
        0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
        0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
        0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
        0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
        0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
        0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
        0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
        0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
        0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
        0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
        0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
        0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
        0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
        0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
        0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
        0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull
    };
    uint64_t w[16], s[8];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = ((uint64_t) m[2 * i] << 32) | m[2 * i + 1];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = ((uint64_t) st[2 * i] << 32) | st[2 * i + 1];
    uint64_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#define TLSREC_CBC_R512(ki)                                                                                 \
    {                                                                                                       \
        const uint64_t t1 = h + (cbc_rotr64(e, 14) ^ cbc_rotr64(e, 18) ^ cbc_rotr64(e, 41)) +               \
                            ((e & f) ^ (~e & g)) + (ki) + w[i];                                             \
        const uint64_t t2 = (cbc_rotr64(a, 28) ^ cbc_rotr64(a, 34) ^ cbc_rotr64(a, 39)) +                   \
                            ((a & b) ^ (a & c) ^ (b & c));                                                  \
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;                                  \
    }
#pragma unroll
    for (int i = 0; i < 16; i++) TLSREC_CBC_R512(K[i])
#pragma unroll 1
    for (int r = 16; r < 80; r += 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint64_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
            w[i] += (cbc_rotr64(y, 19) ^ cbc_rotr64(y, 61) ^ (y >> 6)) + w[(i + 9) & 15] +
                    (cbc_rotr64(x, 1) ^ cbc_rotr64(x, 8) ^ (x >> 7));
            TLSREC_CBC_R512(K[r + i])
        }
    }
#undef TLSREC_CBC_R512
    s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        st[2 * i] = (uint32_t) (s[i] >> 32);
        st[2 * i + 1] = (uint32_t) s[i];
    }
}

/* HMAC midstates of one key (RFC 2104): the state after the key ^ ipad block
 * and after the key ^ opad block; key_len <= 48 < the block size, so the key
 * is never hashed first.  ms: CBC_MS_WORDS words. */
template <int MAC>
TLSREC_CBC_HD void cbc_hmac_midstates(const uint8_t *key, uint32_t *ms)
{
    using H = CbcHash<MAC>;
    const uint32_t klen = cbc_maclen(MAC);
    for (int side = 0; side < 2; side++) {
        const uint32_t padb = side ? 0x5cu : 0x36u;
        uint32_t m[H::B / 4];
        for (int i = 0; i < H::B / 4; i++) {
            uint32_t v = 0;
            for (int j = 0; j < 4; j++) {
                const uint32_t k = 4 * i + j;
                v = (v << 8) | ((k < klen ? key[k] : 0u) ^ padb);
            }
            m[i] = v;
        }
        uint32_t st[H::NS];
        cbc_hash_iv(CbcTag<MAC>(), st);
        cbc_compress(CbcTag<MAC>(), st, m);
        for (int i = 0; i < 16; i++) ms[side * CBC_MS_OUTER + i] = i < H::NS ? st[i] : 0u;
    }
}

/* ---------------- the hashed stream: additional data || record bytes ---- */
/* TLS 1.2 additional data (ssl_extract_add_data_from_record, ssl_msg.c:
 * 568-735): seq || type || version || length (13 bytes), or with a DTLS 1.2
 * connection ID the RFC 9146 form (23 + cid_len bytes).  ctr and cid point
 * into memory, so a byte at a run-time position is a load, not a register
 * array; len_field is a value (in MAC-then-encrypt decryption it depends on
 * the padding). */
struct CbcAad {
    const uint8_t *ctr;
    const uint8_t *cid;
    uint32_t cid_len;
    uint32_t type, ver0, ver1;
    uint32_t len_field;
    uint32_t aad_len;
};

TLSREC_CBC_HD uint32_t cbc_aad_byte(const CbcAad &A, uint32_t k)
{
    if (A.cid_len == 0) {
        if (k < 8) return A.ctr[k];
        return k == 8 ? A.type : k == 9 ? A.ver0 : k == 10 ? A.ver1 : k == 11 ? (A.len_field >> 8) & 0xff
                                                                                : A.len_field & 0xff;
    }
    /* 0xff x 8 || tls12_cid || cid_len || tls12_cid || version || epoch+seq || cid || length */
    if (k < 8) return 0xff;
    if (k >= 13 && k < 21) return A.ctr[k - 13];
    if (k >= 21 && k < 21 + A.cid_len) return A.cid[k - 21];
    return (k == 8 || k == 10) ? A.type : k == 9 ? A.cid_len : k == 11 ? A.ver0 : k == 12 ? A.ver1
           : k == 21 + A.cid_len ? (A.len_field >> 8) & 0xff : A.len_field & 0xff;
}

TLSREC_CBC_HD uint4 cbc_ld16(const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned int v4 __attribute__((ext_vector_type(4)));
    const v4 v = *(const __attribute__((address_space(1))) v4 *) (uintptr_t) p;
    return make_uint4(v.x, v.y, v.z, v.w);
#else
    uint32_t w[4];
    memcpy(w, p, 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
#endif
}

/* 16 bytes of the stream at offset o (a multiple of 16), as little-endian
 * words: bytes below T = aad_len + L are the stream's, byte T is 0x80, the
 * rest zero.  Which path loads them depends on o, aad_len and avail (the
 * readable bytes at `data`) only -- not on L; T enters through masks. */
TLSREC_CBC_HD uint4 cbc_stream_chunk(const CbcAad &A, const uint8_t *data, uint32_t o, uint32_t T, uint32_t avail)
{
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (o >= A.aad_len && o - A.aad_len + 16 <= avail) {
        const uint4 v = cbc_ld16(data + (o - A.aad_len));
        w0 = v.x; w1 = v.y; w2 = v.z; w3 = v.w;
    } else {
#pragma unroll 1
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t k = o + i;
            uint32_t b = 0;
            if (k < A.aad_len) b = cbc_aad_byte(A, k);
            else if (k - A.aad_len < avail) b = data[k - A.aad_len];
            const uint32_t t = b << (8 * (i & 3)), q = i >> 2;
            w0 |= q == 0 ? t : 0u;
            w1 |= q == 1 ? t : 0u;
            w2 |= q == 2 ? t : 0u;
            w3 |= q == 3 ? t : 0u;
        }
    }
    uint32_t w[4] = { w0, w1, w2, w3 };
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int32_t valid = (int32_t) T - (int32_t) (o + 4 * j);   /* stream bytes in this word */
        const uint32_t sh = 8u * ((uint32_t) valid & 3u);
        const uint32_t keep = valid >= 4 ? 0xffffffffu : valid <= 0 ? 0u : (1u << sh) - 1u;
        const uint32_t pad = (valid >= 0 && valid < 4) ? 0x80u << sh : 0u;
        w[j] = (w[j] & keep) | pad;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* HMAC(key of `ms`, additional data || data[0, L)) as DIGW big-endian words.
 *
 * Constant flow in L (mbedtls_ct_hmac, ssl_msg.c:1757): the caller gives
 * maxL >= L and avail >= maxL, both public.  The loop runs the compression
 * for every block of the longest stream (aad_len + maxL), plus once for the
 * outer hash; each block's 16-byte chunks are loaded by cbc_stream_chunk,
 * whose accesses depend on public values only; L enters through byte masks,
 * the position of the 0x80 byte, the length word OR-ed into the block that
 * ends the stream of length L (block fb), and the select that keeps the
 * state after block fb.  With L == maxL the same code is the plain HMAC. */
template <int MAC, typename MS>
TLSREC_CBC_HD void cbc_hmac(uint32_t (&dig)[CbcHash<MAC>::DIGW], MS ms, CbcAad A, const uint8_t *data, uint32_t L,
                            uint32_t maxL, uint32_t avail)
{
    using H = CbcHash<MAC>;
    constexpr int MW = H::B / 4;
    const uint32_t T = A.aad_len + L;
    const uint32_t fb = (T + H::LENB) / H::B;
    const uint32_t nb = (A.aad_len + maxL + H::LENB) / H::B + 1;
    uint32_t st[H::NS], keep[H::NS];
#pragma unroll
    for (int i = 0; i < H::NS; i++) {
        st[i] = ms[i];
        keep[i] = 0;
    }
#pragma unroll 1
    for (uint32_t k = 0; k <= nb; k++) {
        uint32_t m[MW];
        if (k < nb) {
#pragma unroll
            for (int c = 0; c < MW / 4; c++) {
                const uint4 v = cbc_stream_chunk(A, data, k * H::B + 16 * c, T, avail);
                m[4 * c] = cbc_bswap(v.x);
                m[4 * c + 1] = cbc_bswap(v.y);
                m[4 * c + 2] = cbc_bswap(v.z);
                m[4 * c + 3] = cbc_bswap(v.w);
            }
            m[MW - 1] |= k == fb ? (H::B + T) * 8u : 0u;  /* the bit length, ipad block included, ends block fb */
        } else {
            /* outer hash: opad state, then the inner digest as one padded block */
#pragma unroll
            for (int i = 0; i < MW; i++) m[i] = i < H::DIGW ? keep[i] : 0u;
            m[H::DIGW] = 0x80000000u;
            m[MW - 1] = (H::B + 4 * H::DIGW) * 8u;
#pragma unroll
            for (int i = 0; i < H::NS; i++) st[i] = ms[CBC_MS_OUTER + i];
        }
        cbc_compress(CbcTag<MAC>(), st, m);
        const bool last = k == fb;
#pragma unroll
        for (int i = 0; i < H::NS; i++) keep[i] = last ? st[i] : keep[i];
    }
#pragma unroll
    for (int i = 0; i < H::DIGW; i++) dig[i] = st[i];
}

/* ---------------- AES key schedule and inverse cipher -------------------- */
struct CbcSbox {
    uint8_t s[256], inv[256];
    constexpr CbcSbox() : s(), inv()
    {
        uint8_t ex[256] = {}, lg[256] = {};
        uint8_t x = 1;
        for (int i = 0; i < 255; i++) {
            ex[i] = x;
            lg[x] = (uint8_t) i;
            const uint8_t x2 = (uint8_t) ((x << 1) ^ ((x & 0x80) ? 0x1b : 0));
            x = (uint8_t) (x2 ^ x);
        }
        for (int a = 0; a < 256; a++) {
            const uint8_t iv = a ? ex[(255 - lg[a]) % 255] : 0;
            uint8_t v = iv, r = iv;
            for (int k = 0; k < 4; k++) {
                r = (uint8_t) ((r << 1) | (r >> 7));
                v = (uint8_t) (v ^ r);
            }
            s[a] = (uint8_t) (v ^ 0x63);
        }
        for (int a = 0; a < 256; a++) inv[s[a]] = (uint8_t) a;
    }
};

TLSREC_CBC_HD const CbcSbox &cbc_sbox()
{
    static constexpr CbcSbox t{};
    return t;
}

TLSREC_CBC_HD uint32_t cbc_xtime(uint32_t s) { return ((s << 1) ^ (0x1bu & (0u - ((s >> 7) & 1u)))) & 0xff; }
/* s times 9, 11, 13, 14 in GF(2^8) */
TLSREC_CBC_HD void cbc_inv_mults(uint32_t s, uint32_t &m9, uint32_t &mb, uint32_t &md, uint32_t &me)
{
    const uint32_t s2 = cbc_xtime(s), s4 = cbc_xtime(s2), s8 = cbc_xtime(s4);
    m9 = s8 ^ s;
    mb = s8 ^ s2 ^ s;
    md = s8 ^ s4 ^ s;
    me = s8 ^ s4 ^ s2;
}
/* InvMixColumns of one column (bytes a0..a3 from the low byte up) */
TLSREC_CBC_HD uint32_t cbc_inv_mix(uint32_t w)
{
    uint32_t r = 0;
    for (int j = 0; j < 4; j++) {
        uint32_t m9, mb, md, me;
        cbc_inv_mults((w >> (8 * j)) & 0xff, m9, mb, md, me);
        /* input row j feeds output rows j, j+1, j+2, j+3 with 14, 9, 13, 11 */
        const uint32_t col = me | (m9 << 8) | (md << 16) | (mb << 24);
        r ^= j ? cbc_rotl(col, 8 * j) : col;
    }
    return r;
}

/* FIPS-197 5.2 on little-endian column words (as kernels.hip aes_key_expand):
 * rk[4 (nk + 7)] encryption keys; dk the equivalent inverse cipher's
 * (5.3.5: the encryption keys in reverse round order, InvMixColumns applied
 * to the middle rounds). */
TLSREC_CBC_HD void cbc_key_expand(const uint8_t *key, int nk, uint32_t *rk, uint32_t *dk)
{
    const CbcSbox &sb = cbc_sbox();
    const int nr = nk + 6, total = 4 * (nr + 1);
    for (int i = 0; i < nk; i++)
        rk[i] = (uint32_t) key[4 * i] | ((uint32_t) key[4 * i + 1] << 8) | ((uint32_t) key[4 * i + 2] << 16) |
                ((uint32_t) key[4 * i + 3] << 24);
    uint32_t rcon = 1;
    for (int i = nk; i < total; i++) {
        uint32_t t = rk[i - 1];
        if (i % nk == 0) t = (t >> 8) | (t << 24);
        if (i % nk == 0 || (nk > 6 && i % nk == 4))
            t = (uint32_t) sb.s[t & 0xff] | ((uint32_t) sb.s[(t >> 8) & 0xff] << 8) |
                ((uint32_t) sb.s[(t >> 16) & 0xff] << 16) | ((uint32_t) sb.s[t >> 24] << 24);
        if (i % nk == 0) {
            t ^= rcon;
            rcon = cbc_xtime(rcon);
        }
        rk[i] = rk[i - nk] ^ t;
    }
    for (int r = 0; r <= nr; r++)
        for (int c = 0; c < 4; c++) {
            const uint32_t v = rk[4 * (nr - r) + c];
            dk[4 * r + c] = (r == 0 || r == nr) ? v : cbc_inv_mix(v);
        }
}

/* Decryption tables in LDS, the layout of aes_fill_tables (tlsrec_device.h):
 * entry x of table j (0: Td0 = (14 s, 9 s, 13 s, 11 s) with s = InvSbox[x],
 * 1: Td1 = rotl8(Td0)), copy c at lds + x * 256 + j * 128 + c * 4; a lane
 * reads copy (lane & 31), so 32 lanes hit 32 banks whatever their indices.
 * Td2 / Td3 are a 16-bit rotate of Td0 / Td1, and InvSbox[x] is the XOR of
 * the four bytes of Td0[x] (14 ^ 9 ^ 13 ^ 11 = 1), so the last round needs no
 * third table. */
TLSREC_CBC_HD void cbc_fill_dec_tables(uint8_t *lds, int tid, int nthreads)
{
    const CbcSbox &sb = cbc_sbox();
    for (int t = tid; t < 256 * 4; t += nthreads) {
        const uint32_t x = t & 255, part = t >> 8;
        uint32_t m9, mb, md, me;
        cbc_inv_mults(sb.inv[x], m9, mb, md, me);
        const uint32_t t0 = me | (m9 << 8) | (md << 16) | (mb << 24);
        const uint32_t t1 = cbc_rotl(t0, 8);
        const uint4 v0 = make_uint4(t0, t0, t0, t0), v1 = make_uint4(t1, t1, t1, t1);
        uint8_t *row = lds + x * 256 + part * 32;
        *reinterpret_cast<uint4 *>(row) = v0;
        *reinterpret_cast<uint4 *>(row + 16) = v0;
        *reinterpret_cast<uint4 *>(row + 128) = v1;
        *reinterpret_cast<uint4 *>(row + 144) = v1;
    }
}

/* table word for byte k of w: address (byte << 8) | lanebase, one v_perm */
TLSREC_CBC_HD uint32_t cbc_dlook(const uint8_t *lds, uint32_t w, uint32_t lb, int k, int tab)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t a = __builtin_amdgcn_perm(w, lb, 0x0C0C0000u | ((4u + (uint32_t) k) << 8));
#else
    const uint32_t a = (((w >> (8 * k)) & 0xff) << 8) | (lb & 0xff);
#endif
    return *reinterpret_cast<const uint32_t *>(lds + a + tab * 128);
}

TLSREC_CBC_HD uint32_t cbc_rot16(uint32_t x) { return (x << 16) | (x >> 16); }

/* The equivalent inverse cipher of one block.  dkr: the decryption keys with
 * the middle rounds stored rotated by 16 (SlotState::ark), as aes_encrypt
 * takes its keys: a column is
 *     Td0[a] ^ Td1[b] ^ rot16(Td0[c] ^ Td1[d] ^ rot16(k)),
 * with InvShiftRows taking row r of column c from column c - r. */
template <int NR, typename RK>
TLSREC_CBC_HD uint4 cbc_aes_decrypt(const uint8_t *lds, uint32_t lb, RK dkr, uint4 in)
{
    uint32_t s[4] = { in.x ^ dkr[0], in.y ^ dkr[1], in.z ^ dkr[2], in.w ^ dkr[3] };
#pragma unroll
    for (int r = 1; r < NR; r++) {
        uint32_t t[4];
#pragma unroll
        for (int c = 0; c < 4; c++)
            t[c] = cbc_dlook(lds, s[c], lb, 0, 0) ^ cbc_dlook(lds, s[(c + 3) & 3], lb, 1, 1) ^
                   cbc_rot16(cbc_dlook(lds, s[(c + 2) & 3], lb, 2, 0) ^ cbc_dlook(lds, s[(c + 1) & 3], lb, 3, 1) ^
                             dkr[4 * r + c]);
#pragma unroll
        for (int c = 0; c < 4; c++) s[c] = t[c];
    }
    uint32_t o[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t x = cbc_dlook(lds, s[(c + 4 - k) & 3], lb, k, 0);
            x ^= x >> 16;
            x = (x ^ (x >> 8)) & 0xff;
            v |= x << (8 * k);
        }
        o[c] = v ^ dkr[4 * NR + c];
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

/* ---------------- record sizes (host helpers, ssl_tls.c:7822-7835) ------- */
/* explicit IV + ciphertext (+ MAC) of `inner` plaintext bytes -- the content,
 * or with a connection ID the DTLSInnerPlaintext (ssl_msg.c:874-897) -- under
 * a MAC of ml bytes (ssl_msg.c:906-968, :1080-1253).  The one place this
 * arithmetic lives: cbc_record_len, the send frame kernels (stream.hip) and
 * tlsrec_*_out_size_cbc. */
template <typename T>
TLSREC_CBC_HD T cbc_body_len(T ml, bool etm, T inner)
{
    const T body = inner + (etm ? (T) 0 : ml);
    const T padded = (body + 16) & ~(T) 15;         /* 1..16 bytes of padding */
    return 16 + padded + (etm ? ml : (T) 0);
}

/* explicit IV + ciphertext (+ MAC) of a record of content_len bytes */
TLSREC_CBC_HD uint32_t cbc_record_len(int mac, int etm, uint32_t content_len)
{
    const uint32_t ml = cbc_maclen(mac);
    if (ml == 0 || etm < 0 || etm > 1) return 0;
    return cbc_body_len<uint32_t>(ml, etm != 0, content_len);
}

} /* namespace tlsrec */

#endif /* TLSREC_CBC_H */
