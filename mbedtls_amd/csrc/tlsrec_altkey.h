/*
 * tlsrec_altkey.h -- key schedules of the S-box image block ciphers (ARIA,
 * RFC 5794; Camellia, RFC 3713), one lane each: what a slot's key setup runs
 * once per key (kernels.hip for the GCM / CCM slots, cbc_alt.hip for the CBC
 * ones).
 *
 *   - the key expansions and byte-wise / 64-bit-word block functions, as the
 *     AEAD key setup has always run them (`sb`: the cipher's four S-boxes as
 *     4 x 256 bytes, AriaSboxGen / CamSboxGen of tlsrec_device.h);
 *   - the decryption key arrays of both ciphers, on the word layout of
 *     SlotState::ark.  Both ciphers decrypt with their forward function under
 *     a derived key array, so the record kernels hold no inverse cipher.
 *
 * Everything is __host__ __device__, so a host program can check it against
 * a reference implementation (tests/c/alt_keys.cpp).
 */
#ifndef TLSREC_ALTKEY_H
#define TLSREC_ALTKEY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tlsrec_device.h"

namespace tlsrec {

#define TLSREC_ALTKEY_HD __host__ __device__ inline

/* ARIA key schedule and byte-wise block (RFC 5794 2.2, 2.3), one lane:
 * only for the round keys and H = E_K(0^128) of a slot. */
TLSREC_ALTKEY_HD void aria_round_bytes(const uint8_t *sb, uint8_t d[16], const uint8_t rk[16], bool odd, bool diffuse)
{
    uint32_t x[16], y[16];
    for (int i = 0; i < 16; i++) {
        const int t = odd ? (i & 3) : ((i & 3) ^ 2);
        x[i] = sb[t * 256 + (d[i] ^ rk[i])];
    }
    if (diffuse) {
        TLSREC_ARIA_A(y, x);
        for (int i = 0; i < 16; i++) d[i] = (uint8_t) y[i];
    } else {
        for (int i = 0; i < 16; i++) d[i] = (uint8_t) x[i];
    }
}

TLSREC_ALTKEY_HD int aria_key_expand(const uint8_t *sb, const uint8_t *key, int keylen, uint8_t ek[17][16])
{
    const uint8_t C[3][16] = {
        { 0x51, 0x7c, 0xc1, 0xb7, 0x27, 0x22, 0x0a, 0x94, 0xfe, 0x13, 0xab, 0xe8, 0xfa, 0x9a, 0x6e, 0xe0 },
        { 0x6d, 0xb1, 0x4a, 0xcc, 0x9e, 0x21, 0xc8, 0x20, 0xff, 0x28, 0xb1, 0xd5, 0xef, 0x5d, 0xe2, 0xb0 },
        { 0xdb, 0x92, 0x37, 0x1d, 0x21, 0x26, 0xe9, 0x70, 0x03, 0x24, 0x97, 0x75, 0x04, 0xe8, 0xc9, 0x0e },
    };
    const int first = keylen == 16 ? 0 : keylen == 24 ? 1 : 2, nr = keylen / 4 + 8;
    uint8_t w[4][16], t[16], kr[16];
    for (int i = 0; i < 16; i++) { w[0][i] = key[i]; kr[i] = 16 + i < keylen ? key[16 + i] : 0; }
    for (int i = 0; i < 16; i++) t[i] = w[0][i];
    aria_round_bytes(sb, t, C[first], true, true);
    for (int i = 0; i < 16; i++) w[1][i] = t[i] ^ kr[i];
    for (int i = 0; i < 16; i++) t[i] = w[1][i];
    aria_round_bytes(sb, t, C[(first + 1) % 3], false, true);
    for (int i = 0; i < 16; i++) w[2][i] = t[i] ^ w[0][i];
    for (int i = 0; i < 16; i++) t[i] = w[2][i];
    aria_round_bytes(sb, t, C[(first + 2) % 3], true, true);
    for (int i = 0; i < 16; i++) w[3][i] = t[i] ^ w[1][i];
    const int rot[5] = { 19, 31, 128 - 61, 128 - 31, 128 - 19 };   /* right rotations */
    for (int e = 0; e < nr + 1; e++) {
        const uint8_t *a = w[e % 4], *b = w[(e % 4 + 1) % 4];
        const int n = rot[e / 4], by = n / 8, bi = n % 8;
        for (int i = 0; i < 16; i++) {
            const uint8_t hi = b[(i - by + 16) % 16], lo = b[(i - by - 1 + 32) % 16];
            const uint8_t r = (uint8_t) (bi ? ((hi >> bi) | (lo << (8 - bi))) : hi);
            ek[e][i] = a[i] ^ r;
        }
    }
    return nr;
}

TLSREC_ALTKEY_HD void aria_encrypt_bytes(const uint8_t *sb, const uint8_t ek[17][16], int nr, uint8_t st[16])
{
    for (int r = 1; r < nr; r++) aria_round_bytes(sb, st, ek[r - 1], (r & 1) != 0, true);
    aria_round_bytes(sb, st, ek[nr - 1], false, false);
    for (int i = 0; i < 16; i++) st[i] ^= ek[nr][i];
}

/* Camellia key schedule and 64-bit-word block (RFC 3713 2.2-2.4), one lane:
 * only for the subkeys and H = E_K(0^128) of a slot. */
TLSREC_ALTKEY_HD uint64_t cam_f64(const uint8_t *sb, uint64_t x, uint64_t k)
{
    x ^= k;
    const uint32_t xh = (uint32_t) (x >> 32), xl = (uint32_t) x;
    const uint32_t A = ((uint32_t) sb[0 * 256 + (xh >> 24)] << 24) | ((uint32_t) sb[1 * 256 + ((xh >> 16) & 0xff)] << 16) |
                       ((uint32_t) sb[2 * 256 + ((xh >> 8) & 0xff)] << 8) | sb[3 * 256 + (xh & 0xff)];
    const uint32_t B = ((uint32_t) sb[1 * 256 + (xl >> 24)] << 24) | ((uint32_t) sb[2 * 256 + ((xl >> 16) & 0xff)] << 16) |
                       ((uint32_t) sb[3 * 256 + ((xl >> 8) & 0xff)] << 8) | sb[0 * 256 + (xl & 0xff)];
    /* P-layer as in cam_f (tlsrec_device.h) */
    const uint32_t U = A ^ ((B << 8) | (B >> 24));
    const uint32_t V = B ^ ((U << 16) | (U >> 16));
    const uint32_t U2 = U ^ ((V >> 8) | (V << 24));
    return ((uint64_t) (V ^ ((U2 >> 8) | (U2 << 24))) << 32) | U2;
}

TLSREC_ALTKEY_HD void cam_rol128(uint64_t hi, uint64_t lo, int n, uint64_t &oh, uint64_t &ol)
{
    if (n >= 64) { const uint64_t t = hi; hi = lo; lo = t; n -= 64; }
    if (n == 0) { oh = hi; ol = lo; return; }
    oh = (hi << n) | (lo >> (64 - n));
    ol = (lo << n) | (hi >> (64 - n));
}

/* the 26 / 34 subkeys in use order (kw1 kw2 | k1..k6 | ke1 ke2 | ... | kw3 kw4) */
TLSREC_ALTKEY_HD int cam_key_expand(const uint8_t *sb, const uint8_t *key, int keylen, uint64_t sk[34])
{
    const uint64_t SIGMA[6] = { 0xA09E667F3BCC908BULL, 0xB67AE8584CAA73B2ULL, 0xC6EF372FE94F82BEULL,
                                0x54FF53A5F1D36F1CULL, 0x10E527FADE682D1DULL, 0xB05688C2B3E6C1FDULL };
    uint64_t w[4] = { 0, 0, 0, 0 };
    for (int i = 0; i < keylen; i++) w[i / 8] = (w[i / 8] << 8) | key[i];
    if (keylen == 24) w[3] = ~w[2];
    /* src: 0 KL, 1 KR, 2 KA, 3 KB as (hi, lo) */
    uint64_t src[4][2] = { { w[0], w[1] }, { w[2], w[3] }, { 0, 0 }, { 0, 0 } };
    uint64_t d1 = w[0] ^ w[2], d2 = w[1] ^ w[3];
    d2 ^= cam_f64(sb, d1, SIGMA[0]);
    d1 ^= cam_f64(sb, d2, SIGMA[1]);
    d1 ^= w[0];
    d2 ^= w[1];
    d2 ^= cam_f64(sb, d1, SIGMA[2]);
    d1 ^= cam_f64(sb, d2, SIGMA[3]);
    src[2][0] = d1; src[2][1] = d2;
    d1 ^= w[2];
    d2 ^= w[3];
    d2 ^= cam_f64(sb, d1, SIGMA[4]);
    d1 ^= cam_f64(sb, d2, SIGMA[5]);
    src[3][0] = d1; src[3][1] = d2;
    /* (source, rotation, halves: 3 both, 1 high, 2 low), RFC 3713 2.2 */
    const uint8_t s128[14][3] = { { 0, 0, 3 }, { 2, 0, 3 }, { 0, 15, 3 }, { 2, 15, 3 }, { 2, 30, 3 },
                                  { 0, 45, 3 }, { 2, 45, 1 }, { 0, 60, 2 }, { 2, 60, 3 }, { 0, 77, 3 },
                                  { 0, 94, 3 }, { 2, 94, 3 }, { 0, 111, 3 }, { 2, 111, 3 } };
    const uint8_t s256[17][3] = { { 0, 0, 3 }, { 3, 0, 3 }, { 1, 15, 3 }, { 2, 15, 3 }, { 1, 30, 3 },
                                  { 3, 30, 3 }, { 0, 45, 3 }, { 2, 45, 3 }, { 0, 60, 3 }, { 1, 60, 3 },
                                  { 3, 60, 3 }, { 0, 77, 3 }, { 2, 77, 3 }, { 1, 94, 3 }, { 2, 94, 3 },
                                  { 0, 111, 3 }, { 3, 111, 3 } };
    const int rows = keylen == 16 ? 14 : 17;
    int n = 0;
    for (int i = 0; i < rows; i++) {
        const uint8_t *e = keylen == 16 ? s128[i] : s256[i];
        uint64_t h, l;
        cam_rol128(src[e[0]][0], src[e[0]][1], e[1], h, l);
        if (e[2] & 1) sk[n++] = h;
        if (e[2] & 2) sk[n++] = l;
    }
    for (int i = n; i < 34; i++) sk[i] = 0;
    return keylen == 16 ? 18 : 24;
}

TLSREC_ALTKEY_HD void cam_encrypt_u64(const uint8_t *sb, const uint64_t sk[34], int nr, uint64_t &hi, uint64_t &lo)
{
    uint64_t d1 = hi ^ sk[0], d2 = lo ^ sk[1];
    int i = 2;
    const int groups = nr / 6;
    for (int g = 0; g < groups; g++) {
        for (int r = 0; r < 3; r++) {
            d2 ^= cam_f64(sb, d1, sk[i++]);
            d1 ^= cam_f64(sb, d2, sk[i++]);
        }
        if (g != groups - 1) {
            uint32_t x1 = (uint32_t) (d1 >> 32), x2 = (uint32_t) d1;
            uint32_t k1 = (uint32_t) (sk[i] >> 32), k2 = (uint32_t) sk[i];
            uint32_t t = x1 & k1;
            x2 ^= (t << 1) | (t >> 31);
            x1 ^= x2 | k2;
            d1 = ((uint64_t) x1 << 32) | x2;
            i++;
            uint32_t y1 = (uint32_t) (d2 >> 32), y2 = (uint32_t) d2;
            k1 = (uint32_t) (sk[i] >> 32); k2 = (uint32_t) sk[i];
            y1 ^= y2 | k2;
            t = y1 & k1;
            y2 ^= (t << 1) | (t >> 31);
            d2 = ((uint64_t) y1 << 32) | y2;
            i++;
        }
    }
    hi = d2 ^ sk[i];
    lo = d1 ^ sk[i + 1];
}

/* ---------------- decryption keys ---------------------------------------- */
constexpr int ALT_KEY_WORDS = 68;   /* SlotState::ark: 17 ARIA round keys, or 34 Camellia subkeys */

/* ARIA (RFC 5794 2.2): dk1 = ek(n+1), dk i = A(ek(n+2-i)) for i = 2..n,
 * dk(n+1) = ek1 -- the forward cipher under dk is the inverse cipher under ek
 * (A is an involution and SL2 the inverse of SL1).  ek / dk: the nr + 1 round
 * keys as 4 little-endian words each, dk zero beyond them. */
TLSREC_ALTKEY_HD void aria_dec_keys(const uint32_t *ek, int nr, uint32_t *dk)
{
    for (int c = 0; c < 4; c++) {
        dk[c] = ek[4 * nr + c];
        dk[4 * nr + c] = ek[c];
    }
    for (int r = 1; r < nr; r++) {
        uint32_t x[16], y[16];
        for (int i = 0; i < 16; i++) x[i] = (ek[4 * (nr - r) + (i >> 2)] >> (8 * (i & 3))) & 0xffu;
        TLSREC_ARIA_A(y, x);
        for (int c = 0; c < 4; c++)
            dk[4 * r + c] = y[4 * c] | (y[4 * c + 1] << 8) | (y[4 * c + 2] << 16) | (y[4 * c + 3] << 24);
    }
    for (int i = 4 * (nr + 1); i < ALT_KEY_WORDS; i++) dk[i] = 0;
}

/* Camellia (RFC 3713 2.3): the subkeys in reverse order -- the whitening
 * pairs swapped (kw1 kw2 <-> kw3 kw4), the round and FL keys between them
 * reversed as one run (k1 <-> k18 / k24, ke1 <-> ke4 / ke6, ...).  ek / dk:
 * the 26 (nr 18) / 34 (nr 24) 64-bit subkeys in use order as (high, low)
 * words, dk zero beyond them. */
TLSREC_ALTKEY_HD void cam_dec_keys(const uint32_t *ek, int nr, uint32_t *dk)
{
    const int n = nr == 18 ? 26 : 34;
    for (int j = 0; j < n; j++) {
        const int s = j < 2 ? n - 2 + j : j >= n - 2 ? j - (n - 2) : n - 1 - j;
        dk[2 * j] = ek[2 * s];
        dk[2 * j + 1] = ek[2 * s + 1];
    }
    for (int i = 2 * n; i < ALT_KEY_WORDS; i++) dk[i] = 0;
}

} /* namespace tlsrec */

#endif /* TLSREC_ALTKEY_H */
