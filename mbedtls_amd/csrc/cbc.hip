/*
 * cbc.hip -- CBC + HMAC record protection for TLS 1.2 / DTLS 1.2 (AES here,
 * ARIA and Camellia through the same kernel template in cbc_alt.hip): the
 * MBEDTLS_SSL_MODE_CBC (MAC-then-encrypt) and MBEDTLS_SSL_MODE_CBC_ETM
 * (encrypt-then-MAC, RFC 7366) branches of mbedtls_ssl_encrypt_buf
 * (ssl_msg.c:906-968, :1080-1253) and mbedtls_ssl_decrypt_buf (:1435-1702,
 * :1717-1801), for batch records naming a CBC key slot.
 *
 * Shape: that of ccm.hip.  CBC encryption and the hash are each one dependent
 * chain per record, so a record belongs to ONE lane; a 512-thread workgroup
 * holds 512 records and a wave serves its records in key passes over the
 * order the bucket pass built (round keys and HMAC midstates through the
 * constant address space).  One kernel instantiation per (AES rounds, MAC,
 * direction); the MAC order and a DTLS connection ID are wave-uniform
 * run-time branches.  Encryption uses the T-tables of tlsrec_device.h,
 * decryption the Td-tables of tlsrec_cbc.h; both sit in 64 KiB of LDS with a
 * copy per bank.
 *
 * A record is handled in two phases, in the order its slot's MAC order asks
 * for, inside one loop so that each instantiation holds one hash and one
 * cipher call site:
 *   encrypt, MAC-then-encrypt:   hash the plaintext, append MAC and padding; CBC
 *   encrypt, encrypt-then-MAC:   pad, CBC; hash IV || ciphertext, append MAC
 *   decrypt, encrypt-then-MAC:   hash IV || ciphertext and compare BEFORE any
 *                                byte is written; CBC, padding check
 *   decrypt, MAC-then-encrypt:   CBC, padding check; constant-flow hash and
 *                                MAC compare (below)
 *
 * Constant flow of MAC-then-encrypt decryption (ssl_msg.c:1629-1692, :1757):
 * for a given ciphertext length clen and MAC, nothing below depends on the
 * padding length or its validity except through values fed to selects.
 *   1. CBC: clen / 16 iterations, each one 16-byte load and store.
 *   2. padding check: min(256, clen) iterations from clen - min(256, clen),
 *      one byte load each; the count of matching bytes is a sum of compares.
 *   3. cbc_hmac with maxL = clen - maclen (the longest content) and
 *      avail = clen: (aad + maxL + LENB) / B + 2 compressions; every block's
 *      chunks are loaded at addresses fixed by the block index; the content
 *      length L enters as byte masks, the position of the 0x80 byte, the
 *      length word of the block that ends the stream, and the select that
 *      keeps the state after that block.
 *   4. peer MAC: maclen + min(256, maxL) iterations over [min_len, clen), one
 *      byte load each; byte j is compared with digest byte j - L under a
 *      select over the digest words, accumulated into one difference word.
 * The status is formed once, from `correct` and the difference word.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tlsrec.h"
#include "tlsrec_cbc.h"
#include "tlsrec_cbc_kernel.h"
#include "tlsrec_device.h"
#include "tlsrec_frame.h"
#include "tlsrec_internal.h"
#include "tlsrec_recdev.h"

namespace tlsrec {

/* The framing layers (stream, DTLS) do not take CBC slots: their batches run
 * without the CBC kernels, and this kernel gives every record naming a CBC
 * slot the result of a record naming a slot that was never loaded -- and
 * writes that result for the unusable slots too: in a table of CBC keys only
 * no AEAD kernel runs that would flag them. */
__global__ __launch_bounds__(256) void tlsrec_cbc_refuse_kernel(CbcArgs a)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t s = a.recs[i].slot;
    const int c = s < a.capacity ? a.slots[s].km.cipher : 0;
    if (c == 0 || cbc_is_cipher(c)) bad_slot_result(a.recs[i], &a.res[i]);
}

/* Zeroize what a CBC key left in slots [first, first + count) that the AEAD
 * key setup does not overwrite: the round keys of both directions (AES:
 * SlotState::rk / rkr and ark; ARIA / Camellia: ark and the decryption key
 * array in rk / rkr) and the HMAC midstates.  One workgroup per slot; slots of
 * other ciphers are left alone.  Runs before the slots' cipher_of entries change. */
__global__ __launch_bounds__(64) void tlsrec_cbc_wipe_kernel(SlotState *slots, uint4 *ghtab, const uint8_t *cipher_of,
                                                             uint32_t first, uint32_t count)
{
    if (blockIdx.x >= count) return;
    const uint32_t slot = first + blockIdx.x;
    if (!cbc_is_cipher(cipher_of[slot])) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < 68; i += 64) slots[slot].ark[i] = 0;
    if (tid < 60) {
        slots[slot].rk[tid] = 0;
        slots[slot].rkr[tid] = 0;
    }
    uint32_t *mw = reinterpret_cast<uint32_t *>(ghtab + (size_t) slot * KEY_TABLE_WORDS);
    if (tid < CBC_MS_WORDS) mw[tid] = 0;
}

/* Key setup of CBC slots: one workgroup per slot; lane 0 expands the AES keys
 * of both directions and the HMAC midstates into LDS, the workgroup stores
 * them: SlotState::rk / rkr (encryption), ::ark (decryption, middle rounds
 * rotated as rkr), the midstates at the head of the slot's GHASH table area;
 * the rest of that area (an earlier GCM key's tables of H) is zeroized. */
__global__ __launch_bounds__(64) void tlsrec_cbc_keysetup_kernel(SlotState *slots, uint4 *ghtab, uint8_t *cipher_of,
                                                                 const tlsrec_cbc_key_material *keys, uint32_t first,
                                                                 uint32_t count)
{
    __shared__ uint32_t rk[64], dk[64], ms[CBC_MS_WORDS];
    if (blockIdx.x >= count) return;
    const uint32_t slot = first + blockIdx.x;
    const tlsrec_cbc_key_material *k = &keys[blockIdx.x];
    SlotState *st = &slots[slot];
    const int tid = threadIdx.x;
    const int cipher = k->cipher, mac = k->mac;
    const int nk = (int) cbc_aes_keylen(cipher) / 4, nr = nk + 6;
    if (tid == 0) {
        cbc_key_expand(k->key, nk, rk, dk);
        if (mac == TLSREC_MAC_SHA1) cbc_hmac_midstates<TLSREC_MAC_SHA1>(k->mac_key, ms);
        else if (mac == TLSREC_MAC_SHA256) cbc_hmac_midstates<TLSREC_MAC_SHA256>(k->mac_key, ms);
        else cbc_hmac_midstates<TLSREC_MAC_SHA384>(k->mac_key, ms);
        tlsrec_key_material km;
        __builtin_memset(&km, 0, sizeof(km));
        km.cipher = (uint8_t) cipher;
        km.tls_minor = 3;
        km.reserved[1] = (uint8_t) mac;       /* [0] mirrors the CID length (tlsrec_keytab_set_cid) */
        km.reserved[2] = k->etm;
        st->km = km;
        for (int i = 0; i < 4 * nk; i++) st->km.key[i] = k->key[i];
        st->nr = (uint32_t) nr;
        st->cid_len = 0;                      /* a (re)load leaves the slot without a CID */
        for (int i = 0; i < 16; i++) {
            st->h[i] = 0;
            st->hpow[i >> 2][i & 3] = 0;
        }
        cipher_of[slot] = (uint8_t) cipher;
    }
    __syncthreads();
    const int total = 4 * (nr + 1);
    for (int i = tid; i < 68; i += 64) {
        const bool used = i < total, middle = i >= 4 && i < 4 * nr;
        if (i < 60) {
            st->rk[i] = used ? rk[i] : 0u;
            st->rkr[i] = used ? (middle ? cbc_rot16(rk[i]) : rk[i]) : 0u;
        }
        st->ark[i] = used ? (middle ? cbc_rot16(dk[i]) : dk[i]) : 0u;
    }
    uint32_t *mw = reinterpret_cast<uint32_t *>(ghtab + (size_t) slot * KEY_TABLE_WORDS);
    if (tid < CBC_MS_WORDS) mw[tid] = ms[tid];
    uint4 *tab = ghtab + (size_t) slot * KEY_TABLE_WORDS;
    for (int i = CBC_MS_WORDS / 4 + tid; i < KEY_TABLE_WORDS; i += 64) tab[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (tid < CBC_MS_WORDS) ms[tid] = 0;     /* key-derived values out of LDS */
    rk[tid] = 0;
    dk[tid] = 0;
}

} /* namespace tlsrec */

using namespace tlsrec;

/* `count` records of ONE kind: alt = 0 AES keys (the kernel above), 1 ARIA or Camellia keys
 * (cbc_alt.hip).  The engine splits a mixed load into runs of one kind. */
extern "C" hipError_t tlsrec__launch_cbc_keysetup(SlotState *slots, uint4 *ghtab, uint8_t *cipher_of,
                                                  const tlsrec_cbc_key_material *keys, uint32_t first, uint32_t count,
                                                  int alt, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    if (alt) return tlsrec__launch_cbc_alt_keysetup(slots, ghtab, cipher_of, keys, first, count, st);
    hipLaunchKernelGGL(tlsrec_cbc_keysetup_kernel, dim3(count), dim3(64), 0, st, slots, ghtab, cipher_of, keys, first,
                       count);
    return hipGetLastError();
}

extern "C" hipError_t tlsrec__launch_cbc_refuse(const CbcArgs *a, hipStream_t st)
{
    if (a->n == 0) return hipSuccess;
    hipLaunchKernelGGL(tlsrec_cbc_refuse_kernel, dim3((uint32_t) ((a->n + 255) / 256)), dim3(256), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t tlsrec__launch_cbc_wipe(SlotState *slots, uint4 *ghtab, const uint8_t *cipher_of, uint32_t first,
                                              uint32_t count, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(tlsrec_cbc_wipe_kernel, dim3(count), dim3(64), 0, st, slots, ghtab, cipher_of, first, count);
    return hipGetLastError();
}

/* variants: bit 3 * (cipher - TLSREC_CIPHER_CBC_FIRST) + (mac - 1) for every
 * (cipher, MAC) pair the table holds; one launch each over the CBC class */
extern "C" hipError_t tlsrec__launch_cbc(const CbcArgs *a, int dec, uint32_t variants, hipStream_t st)
{
    const uint32_t g = (uint32_t) ((a->n + CBC_THREADS - 1) / CBC_THREADS);
    if (g == 0) return hipSuccess;
    hipError_t e = hipSuccess;
#define TLSREC_CBC_LAUNCH(NR, MAC, BIT)                                                                          \
    if (e == hipSuccess && (variants & (1u << (BIT)))) {                                                         \
        if (dec) hipLaunchKernelGGL((tlsrec_cbc_kernel<NR, MAC, true>), dim3(g), dim3(CBC_THREADS), 0, st, *a);  \
        else hipLaunchKernelGGL((tlsrec_cbc_kernel<NR, MAC, false>), dim3(g), dim3(CBC_THREADS), 0, st, *a);     \
        e = hipGetLastError();                                                                                   \
    }
    TLSREC_CBC_LAUNCH(10, TLSREC_MAC_SHA1, 0)
    TLSREC_CBC_LAUNCH(10, TLSREC_MAC_SHA256, 1)
    TLSREC_CBC_LAUNCH(10, TLSREC_MAC_SHA384, 2)
    TLSREC_CBC_LAUNCH(14, TLSREC_MAC_SHA1, 3)
    TLSREC_CBC_LAUNCH(14, TLSREC_MAC_SHA256, 4)
    TLSREC_CBC_LAUNCH(14, TLSREC_MAC_SHA384, 5)
#undef TLSREC_CBC_LAUNCH
    if (e == hipSuccess && (variants >> 6)) e = tlsrec__launch_cbc_alt(a, dec, variants, g, st);   /* ARIA, Camellia */
    return e;
}
