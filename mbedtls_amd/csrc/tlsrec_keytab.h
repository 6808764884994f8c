/*
 * tlsrec_keytab.h -- the key table (keytab.hip).  KeytabBook is what the host knows about the slots; every
 * load, staged commit and slot release goes through its three functions, so the figures the launches are
 * sized from (gcm_plan reads nloaded) cannot drift apart.  Plain C++17 without a HIP include, like
 * tlsrec_plan.h: a host compiler checks it alone (tests/c/keytab_book.cpp).  struct tlsrec_keytab, the book
 * plus the device memory, exists under hipcc only; keytab.hip and batch.hip are the units that see inside it.
 */
#ifndef TLSREC_KEYTAB_H
#define TLSREC_KEYTAB_H

#include <stdint.h>

#include "tlsrec.h"

namespace tlsrec {

static_assert(TLSREC_CIPHER_CBC_LAST < 32 && 3 * (TLSREC_CIPHER_CBC_LAST - TLSREC_CIPHER_CBC_FIRST) + 2 < 32,
              "cipher_mask and cbc_variants are 32-bit words");
/* cipher_mask bits of the CBC + HMAC ciphers (the ids cbc_is_cipher() accepts) */
constexpr uint32_t CBC_CIPHER_BITS = (1u << TLSREC_CIPHER_AES_128_CBC) | (1u << TLSREC_CIPHER_AES_256_CBC) |
                                     (1u << TLSREC_CIPHER_ARIA_128_CBC) | (1u << TLSREC_CIPHER_ARIA_256_CBC) |
                                     (1u << TLSREC_CIPHER_CAMELLIA_128_CBC) | (1u << TLSREC_CIPHER_CAMELLIA_256_CBC);

struct KeytabBook {
    uint32_t capacity;
    uint8_t *h_cipher;        /* [capacity] host mirror of each slot's cipher, 0 = holds no key */
    uint32_t nloaded;         /* slots holding a key */
    uint32_t cipher_mask;     /* 1 << TLSREC_CIPHER_* of every cipher ever loaded */
    uint32_t cbc_variants;    /* CBC slots loaded: cbc_bit(cipher, mac) of each (tlsrec__launch_cbc) */
    uint32_t cbc_etm;         /* ... and bit etm: the MAC orders among them (launch log) */
    /* bit of a (cipher, MAC) pair in cbc_variants: cbc_variant_bit of tlsrec_cbc.h, restated without HIP */
    static constexpr uint32_t cbc_bit(int cipher, int mac)
    {
        return 1u << (3 * (cipher - TLSREC_CIPHER_CBC_FIRST) + (mac - 1));
    }
    /* slots [first, first + count) lie in the table (count = 0 at first = capacity: an empty range) */
    bool holds(uint32_t first, uint32_t count) const { return !(first > capacity || count > capacity - first); }
    /* slots [first, first + count) now hold keys of `cipher` */
    void note(uint32_t first, uint32_t count, int cipher)
    {
        for (uint32_t i = first; i < first + count; i++) {
            if (h_cipher[i] == 0) nloaded++;
            h_cipher[i] = (uint8_t) cipher;
            cipher_mask |= 1u << cipher;
        }
    }
    void note_cbc(uint32_t first, uint32_t count, int cipher, int mac, int etm)
    {
        note(first, count, cipher);
        if (count) {
            cbc_variants |= cbc_bit(cipher, mac);
            cbc_etm |= 1u << etm;
        }
    }
    /* the slot holds no key any more.  Its cipher stays in the masks: a later batch may launch one kernel
     * more, which finds no record */
    void clear(uint32_t slot)
    {
        if (h_cipher[slot] == 0) return;
        h_cipher[slot] = 0;
        nloaded--;
    }
};

} /* namespace tlsrec */

#ifdef __HIPCC__
#include <pthread.h>

#include "tlsrec_internal.h"

struct tlsrec_keytab : tlsrec::KeytabBook {
    int device;
    int cu;                   /* compute units of the device (launch sizing), read once at create */
    tlsrec::SlotState *d_slots;
    uint4 *d_ghtab;
    uint8_t *d_cipher;        /* each slot's cipher, one byte (the bucket pass reads it per record:
                                 an L2-resident array instead of a line of the 1 KiB slot) */
    tlsrec_key_material *d_stage;
    tlsrec_cbc_key_material *d_stage_cbc;   /* capacity records, made by the first CBC batch derivation */
    volatile uint32_t has_cid; /* some slot was given a DTLS connection ID: launch the CID kernels */
    uint8_t *d_dummy;         /* GcmArgs::dummy: 64 KiB the idle lanes of a wave-pass round load and store */
    HostPipe *pipe;           /* tlsrec_host_batch_* (host_pipe.hip), made on first use under pipe_mu */
    pthread_mutex_t pipe_mu;
};
#endif

#endif
