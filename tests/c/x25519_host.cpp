/*
 * x25519_host: the ladder of mbedtls_amd/csrc/tlsrec_x25519.h run on the host,
 * without the library and without a device, under the address and
 * undefined-behaviour sanitizers (tests/test_x25519_cpu.py builds and runs it):
 *   - the RFC 7748 vectors: section 5.2 (both, and the iterated one after 1 and
 *     1 000 iterations) and the section 6.1 exchange;
 *   - the fixed-base form against the general one with u = 9;
 *   - with a file argument, one case per line, "scalar u expected ok" in hex
 *     (the edge set, written by the test from its integer model).
 * The signed limbs must never overflow or be shifted left while negative: that
 * is what the undefined-behaviour sanitizer watches here.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tlsrec_x25519.h"

static int failures = 0;

static void unhex(const char *s, uint8_t out[32])
{
    if (strlen(s) != 64) {
        fprintf(stderr, "FAIL: bad hex length %zu\n", strlen(s));
        exit(2);
    }
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) {
            fprintf(stderr, "FAIL: bad hex\n");
            exit(2);
        }
        out[i] = (uint8_t) v;
    }
}

static void words(const uint8_t b[32], uint32_t (&w)[8])
{
    for (int j = 0; j < 8; j++)
        w[j] = (uint32_t) b[4 * j] | ((uint32_t) b[4 * j + 1] << 8) | ((uint32_t) b[4 * j + 2] << 16) |
               ((uint32_t) b[4 * j + 3] << 24);
}

template <bool BASE> static uint32_t run(uint8_t out[32], const uint8_t k[32], const uint8_t u[32])
{
    uint32_t kw[8], uw[8], rw[8];
    words(k, kw);
    words(u, uw);
    const uint32_t ok = tlsrec::x25519<BASE>(rw, kw, uw);
    for (int j = 0; j < 32; j++) out[j] = (uint8_t) (rw[j >> 2] >> (8 * (j & 3)));
    return ok;
}

static void expect(const char *what, const uint8_t got[32], const uint8_t want[32])
{
    if (memcmp(got, want, 32) != 0) {
        fprintf(stderr, "FAIL: %s\n", what);
        failures++;
    }
}

static void vector(const char *what, const char *k, const char *u, const char *r)
{
    uint8_t kb[32], ub[32], rb[32], out[32];
    unhex(k, kb);
    unhex(u, ub);
    unhex(r, rb);
    if (run<false>(out, kb, ub) != 1) {
        fprintf(stderr, "FAIL: %s: ok\n", what);
        failures++;
    }
    expect(what, out, rb);
}

int main(int argc, char **argv)
{
    vector("RFC 7748 5.2 vector 1", "a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
           "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
           "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552");
    vector("RFC 7748 5.2 vector 2", "4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
           "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
           "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957");
    const char *apriv = "77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a";
    const char *apub = "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a";
    const char *bpriv = "5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb";
    const char *bpub = "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f";
    const char *shared = "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742";
    const char *nine = "0900000000000000000000000000000000000000000000000000000000000000";
    vector("RFC 7748 6.1 Alice's public key", apriv, nine, apub);
    vector("RFC 7748 6.1 Bob's public key", bpriv, nine, bpub);
    vector("RFC 7748 6.1 Alice's shared secret", apriv, bpub, shared);
    vector("RFC 7748 6.1 Bob's shared secret", bpriv, apub, shared);

    /* the fixed-base form is the general one at u = 9 (its u argument is not looked at) */
    {
        uint8_t k[32], u9[32], junk[32], a[32], b[32];
        unhex(nine, u9);
        memset(junk, 0xa5, 32);
        for (int t = 0; t < 16; t++) {
            for (int i = 0; i < 32; i++) k[i] = (uint8_t) (37 * t + 101 * i + (i * i) % 13);
            run<true>(a, k, junk);
            run<false>(b, k, u9);
            expect("fixed base", a, b);
        }
    }

    /* the iterated vector: k, u = X25519(k, u), k */
    {
        uint8_t k[32], u[32], r[32], want[32];
        unhex(nine, k);
        unhex(nine, u);
        for (int it = 1; it <= 1000; it++) {
            run<false>(r, k, u);
            memcpy(u, k, 32);
            memcpy(k, r, 32);
            if (it == 1) {
                unhex("422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079", want);
                expect("RFC 7748 5.2 after 1 iteration", k, want);
            }
        }
        unhex("684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51", want);
        expect("RFC 7748 5.2 after 1 000 iterations", k, want);
    }

    int cases = 0;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) {
            fprintf(stderr, "FAIL: cannot open %s\n", argv[1]);
            return 2;
        }
        char ks[80], us[80], rs[80];
        unsigned okw = 0;
        while (fscanf(f, "%79s %79s %79s %u", ks, us, rs, &okw) == 4) {
            uint8_t k[32], u[32], want[32], out[32];
            unhex(ks, k);
            unhex(us, u);
            unhex(rs, want);
            const uint32_t ok = run<false>(out, k, u);
            if (ok != okw || memcmp(out, want, 32) != 0) {
                fprintf(stderr, "FAIL: case %d: k %s u %s\n", cases, ks, us);
                failures++;
            }
            cases++;
        }
        fclose(f);
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("x25519_host ok: RFC vectors, %d file cases\n", cases);
    return 0;
}
