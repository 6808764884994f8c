/*
 * alt_keys: the decryption key arrays of ARIA and Camellia
 * (mbedtls_amd/csrc/tlsrec_altkey.h: aria_dec_keys, cam_dec_keys) checked on
 * the host, without a device.  For the RFC vectors and 1 000 seeded random
 * keys per key size:
 *   - the forward cipher under the derived decryption keys inverts the forward
 *     cipher under the encryption keys;
 *   - forward / inverse equal OpenSSL's EVP ECB encryption / decryption.
 * The block functions are the header's own byte-wise / 64-bit-word ones (the
 * key setup's), run here as host code.  Built with the address and
 * undefined-behaviour sanitizers (`make check_alt_keys`).
 */
#include <openssl/evp.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tlsrec_altkey.h"

using namespace tlsrec;

static const AriaSboxGen kAria{};
static const CamSboxGen kCam{};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint8_t rng_byte(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint8_t) (rng_state >> 32);
}

static void die(const char *what, int cam, int keylen, int iter)
{
    fprintf(stderr, "FAIL: %s (%s-%d, key %d)\n", what, cam ? "camellia" : "aria", 8 * keylen, iter);
    exit(1);
}

static void evp_ecb(const EVP_CIPHER *c, const uint8_t *key, const uint8_t in[16], uint8_t out[16], int enc)
{
    EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
    int n = 0;
    if (!ctx || EVP_CipherInit_ex(ctx, c, NULL, key, NULL, enc) != 1 || EVP_CIPHER_CTX_set_padding(ctx, 0) != 1 ||
        EVP_CipherUpdate(ctx, out, &n, in, 16) != 1 || n != 16) {
        fprintf(stderr, "FAIL: EVP\n");
        exit(1);
    }
    EVP_CIPHER_CTX_free(ctx);
}

/* one block under a key array in the slot's word layout */
static void aria_block(const uint32_t *kw, int nr, uint8_t st[16])
{
    uint8_t kb[17][16];
    memset(kb, 0, sizeof(kb));
    for (int e = 0; e <= nr; e++)
        for (int i = 0; i < 16; i++) kb[e][i] = (uint8_t) (kw[4 * e + (i >> 2)] >> (8 * (i & 3)));
    aria_encrypt_bytes(&kAria.v[0][0], kb, nr, st);
}

static void cam_block(const uint32_t *kw, int nr, uint8_t st[16])
{
    uint64_t sk[34], hi = 0, lo = 0;
    for (int i = 0; i < 34; i++) sk[i] = ((uint64_t) kw[2 * i] << 32) | kw[2 * i + 1];
    for (int i = 0; i < 8; i++) {
        hi = (hi << 8) | st[i];
        lo = (lo << 8) | st[8 + i];
    }
    cam_encrypt_u64(&kCam.v[0][0], sk, nr, hi, lo);
    for (int i = 0; i < 8; i++) {
        st[i] = (uint8_t) (hi >> (56 - 8 * i));
        st[8 + i] = (uint8_t) (lo >> (56 - 8 * i));
    }
}

static void check(int cam, const uint8_t *key, int keylen, const uint8_t pt[16], const uint8_t *want_ct, int iter)
{
    uint32_t ek[ALT_KEY_WORDS], dk[ALT_KEY_WORDS];
    int nr;
    memset(ek, 0, sizeof(ek));
    memset(dk, 0xa5, sizeof(dk));
    if (cam) {
        uint64_t sk[34];
        nr = cam_key_expand(&kCam.v[0][0], key, keylen, sk);
        for (int i = 0; i < 34; i++) {
            ek[2 * i] = (uint32_t) (sk[i] >> 32);
            ek[2 * i + 1] = (uint32_t) sk[i];
        }
        cam_dec_keys(ek, nr, dk);
    } else {
        uint8_t eb[17][16];
        nr = aria_key_expand(&kAria.v[0][0], key, keylen, eb);
        for (int e = 0; e <= nr; e++)
            for (int c = 0; c < 4; c++)
                ek[4 * e + c] = (uint32_t) eb[e][4 * c] | ((uint32_t) eb[e][4 * c + 1] << 8) |
                                ((uint32_t) eb[e][4 * c + 2] << 16) | ((uint32_t) eb[e][4 * c + 3] << 24);
        aria_dec_keys(ek, nr, dk);
    }
    const int used = cam ? (nr == 18 ? 52 : 68) : 4 * (nr + 1);
    for (int i = used; i < ALT_KEY_WORDS; i++)
        if (dk[i] != 0) die("decryption key words past the schedule are not zero", cam, keylen, iter);
    const EVP_CIPHER *c = cam ? (keylen == 16 ? EVP_camellia_128_ecb() : EVP_camellia_256_ecb())
                              : (keylen == 16 ? EVP_aria_128_ecb() : EVP_aria_256_ecb());
    uint8_t ct[16], back[16], ref[16];
    memcpy(ct, pt, 16);
    cam ? cam_block(ek, nr, ct) : aria_block(ek, nr, ct);
    evp_ecb(c, key, pt, ref, 1);
    if (memcmp(ct, ref, 16) != 0) die("forward cipher differs from EVP", cam, keylen, iter);
    if (want_ct && memcmp(ct, want_ct, 16) != 0) die("forward cipher differs from the RFC vector", cam, keylen, iter);
    memcpy(back, ct, 16);
    cam ? cam_block(dk, nr, back) : aria_block(dk, nr, back);
    if (memcmp(back, pt, 16) != 0) die("decryption keys do not invert the forward cipher", cam, keylen, iter);
    /* and on a block that is no ciphertext of ours */
    uint8_t x[16], y[16];
    for (int i = 0; i < 16; i++) x[i] = rng_byte();
    memcpy(y, x, 16);
    cam ? cam_block(dk, nr, y) : aria_block(dk, nr, y);
    evp_ecb(c, key, x, ref, 0);
    if (memcmp(y, ref, 16) != 0) die("decryption differs from EVP", cam, keylen, iter);
}

static void hex(const char *s, uint8_t *out)
{
    for (size_t i = 0; s[2 * i]; i++) {
        unsigned v;
        sscanf(s + 2 * i, "%2x", &v);
        out[i] = (uint8_t) v;
    }
}

int main(void)
{
    uint8_t key[32], pt[16], ct[16];
    /* RFC 5794 Appendix A.1, A.3 */
    for (int i = 0; i < 32; i++) key[i] = (uint8_t) i;
    hex("00112233445566778899aabbccddeeff", pt);
    hex("d718fbd6ab644c739da95f3be6451778", ct);
    check(0, key, 16, pt, ct, -1);
    hex("f92bd7c79fb72e2f2b8f80c1972d24fc", ct);
    check(0, key, 32, pt, ct, -1);
    /* RFC 3713 Appendix A */
    hex("0123456789abcdeffedcba987654321000112233445566778899aabbccddeeff", key);
    hex("0123456789abcdeffedcba9876543210", pt);
    hex("67673138549669730857065648eabe43", ct);
    check(1, key, 16, pt, ct, -1);
    hex("9acc237dff16d76c20ef7c919e3a7509", ct);
    check(1, key, 32, pt, ct, -1);
    int n = 4;
    for (int cam = 0; cam < 2; cam++)
        for (int keylen = 16; keylen <= 32; keylen += 16)
            for (int it = 0; it < 1000; it++, n++) {
                for (int i = 0; i < 32; i++) key[i] = rng_byte();
                for (int i = 0; i < 16; i++) pt[i] = rng_byte();
                check(cam, key, keylen, pt, NULL, it);
            }
    printf("alt_keys: %d keys ok\n", n);
    return 0;
}
