/*
 * keytab_book -- the key table's host bookkeeping (mbedtls_amd/csrc/tlsrec_keytab.h KeytabBook) against a
 * model kept beside it, under -fsanitize=address,undefined (tests/c/Makefile keytab_book): note / note_cbc /
 * clear over a table of 8 slots, every figure compared after every step, and the range check at its edges.
 * Host only: no library, no device.  Exit status 0 = every check held.
 */
#include <stdio.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_keytab.h"

using tlsrec::KeytabBook;

static int fails = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond) && fails++ < 20) {        \
            fprintf(stderr, "%s: ", #cond);   \
            fprintf(stderr, __VA_ARGS__);     \
            fputc('\n', stderr);              \
        }                                     \
    } while (0)

constexpr uint32_t CAP = 8;

/* what the book must say, kept the slow way */
struct Model {
    uint8_t cipher[CAP] = {};
    uint32_t ever = 0, variants = 0, etm = 0;
};

/* the documented layout of cbc_variants: three MAC bits per CBC cipher id */
static uint32_t variant_bit(int cipher, int mac) { return 1u << (3 * (cipher - TLSREC_CIPHER_CBC_FIRST) + (mac - 1)); }

static void compare(const KeytabBook &b, const Model &m, const char *step)
{
    uint32_t loaded = 0;
    for (uint32_t i = 0; i < CAP; i++) loaded += b.h_cipher[i] != 0;
    CHECK(b.nloaded == loaded, "%s: nloaded=%u, %u slots hold a cipher", step, b.nloaded, loaded);
    CHECK(memcmp(b.h_cipher, m.cipher, CAP) == 0, "%s: h_cipher", step);
    CHECK(b.cipher_mask == m.ever, "%s: cipher_mask=%#x want %#x", step, b.cipher_mask, m.ever);
    CHECK(b.cbc_variants == m.variants, "%s: cbc_variants=%#x want %#x", step, b.cbc_variants, m.variants);
    CHECK(b.cbc_etm == m.etm, "%s: cbc_etm=%#x want %#x", step, b.cbc_etm, m.etm);
    CHECK(b.capacity == CAP, "%s: capacity=%u", step, b.capacity);
}

static void note(KeytabBook &b, Model &m, uint32_t first, uint32_t count, int cipher, const char *step)
{
    b.note(first, count, cipher);
    for (uint32_t i = first; i < first + count; i++) m.cipher[i] = (uint8_t) cipher;
    if (count) m.ever |= 1u << cipher;
    compare(b, m, step);
}

static void note_cbc(KeytabBook &b, Model &m, uint32_t first, uint32_t count, int cipher, int mac, int etm,
                     const char *step)
{
    b.note_cbc(first, count, cipher, mac, etm);
    for (uint32_t i = first; i < first + count; i++) m.cipher[i] = (uint8_t) cipher;
    if (count) {
        m.ever |= 1u << cipher;
        m.variants |= variant_bit(cipher, mac);
        m.etm |= 1u << etm;
    }
    compare(b, m, step);
}

static void clear(KeytabBook &b, Model &m, uint32_t slot, const char *step)
{
    b.clear(slot);
    m.cipher[slot] = 0;      /* and nothing else: the masks keep the cipher */
    compare(b, m, step);
}

int main(void)
{
    uint8_t mirror[CAP] = {};
    KeytabBook b = {};
    b.capacity = CAP;
    b.h_cipher = mirror;
    Model m;
    compare(b, m, "empty");

    note(b, m, 0, 3, TLSREC_CIPHER_AES_128_GCM, "three AES-128-GCM slots");
    CHECK(b.nloaded == 3, "nloaded=%u", b.nloaded);
    note(b, m, 1, 1, TLSREC_CIPHER_AES_128_GCM, "the same cipher again on a loaded slot");
    CHECK(b.nloaded == 3, "re-noting raised nloaded to %u", b.nloaded);
    note(b, m, 2, 2, TLSREC_CIPHER_CHACHA20_POLY1305, "another cipher over a loaded and a free slot");
    CHECK(b.nloaded == 4, "nloaded=%u", b.nloaded);
    note(b, m, CAP, 0, TLSREC_CIPHER_AES_256_GCM, "an empty range at the end");
    note(b, m, CAP - 1, 1, TLSREC_CIPHER_AES_256_GCM, "the last slot");

    note_cbc(b, m, 4, 2, TLSREC_CIPHER_AES_128_CBC, TLSREC_MAC_SHA256, 0, "AES-128-CBC + SHA-256, MAC-then-encrypt");
    note_cbc(b, m, 5, 1, TLSREC_CIPHER_AES_256_CBC, TLSREC_MAC_SHA384, 1, "AES-256-CBC + SHA-384, encrypt-then-MAC");
    note_cbc(b, m, 6, 1, TLSREC_CIPHER_CAMELLIA_256_CBC, TLSREC_MAC_SHA384, 1, "the last CBC cipher id");
    note_cbc(b, m, 6, 0, TLSREC_CIPHER_ARIA_128_CBC, TLSREC_MAC_SHA1, 0, "an empty CBC range");
    CHECK(b.nloaded == 8, "nloaded=%u", b.nloaded);
    CHECK(b.cbc_variants == (KeytabBook::cbc_bit(TLSREC_CIPHER_AES_128_CBC, TLSREC_MAC_SHA256) |
                             KeytabBook::cbc_bit(TLSREC_CIPHER_AES_256_CBC, TLSREC_MAC_SHA384) |
                             KeytabBook::cbc_bit(TLSREC_CIPHER_CAMELLIA_256_CBC, TLSREC_MAC_SHA384)),
          "cbc_variants=%#x", b.cbc_variants);
    CHECK(b.cbc_etm == 3u, "cbc_etm=%#x", b.cbc_etm);

    /* a CBC slot reloaded with an AEAD key: the CBC bits stay */
    note(b, m, 4, 1, TLSREC_CIPHER_AES_256_GCM, "an AEAD key over a CBC slot");
    CHECK(b.cipher_mask & (1u << TLSREC_CIPHER_AES_128_CBC), "cipher_mask=%#x", b.cipher_mask);

    const uint32_t before = b.cipher_mask;
    clear(b, m, 2, "clear a loaded slot");
    CHECK(b.nloaded == 7 && b.cipher_mask == before, "nloaded=%u cipher_mask=%#x", b.nloaded, b.cipher_mask);
    clear(b, m, 2, "clear it again");
    CHECK(b.nloaded == 7, "clearing an unloaded slot moved nloaded to %u", b.nloaded);
    clear(b, m, 5, "clear the only AES-256-CBC slot");
    CHECK(b.cipher_mask & (1u << TLSREC_CIPHER_AES_256_CBC), "cipher_mask=%#x", b.cipher_mask);
    note(b, m, 2, 1, TLSREC_CIPHER_AES_128_GCM, "load the cleared slot again");
    CHECK(b.nloaded == 7, "nloaded=%u", b.nloaded);
    for (uint32_t i = 0; i < CAP; i++) clear(b, m, i, "clear every slot");
    CHECK(b.nloaded == 0 && b.cipher_mask == before, "nloaded=%u cipher_mask=%#x", b.nloaded, b.cipher_mask);

    /* the range check */
    CHECK(!b.holds(CAP + 1, 0), "first = capacity + 1");
    CHECK(!b.holds(0xffffffffu, 2), "first = 0xffffffff, count = 2");
    CHECK(!b.holds(0, 0xffffffffu), "count = 0xffffffff");
    CHECK(!b.holds(1, 0xffffffffu), "first = 1, count = 0xffffffff");
    CHECK(!b.holds(CAP, 1), "first = capacity, count = 1");
    CHECK(!b.holds(CAP - 1, 2), "first = capacity - 1, count = 2");
    CHECK(b.holds(CAP, 0), "first = capacity, count = 0");
    CHECK(b.holds(0, CAP), "the whole table");
    CHECK(b.holds(CAP - 1, 1), "the last slot");

    printf("keytab_book: %d failed\n", fails);
    return fails ? 1 : 0;
}
