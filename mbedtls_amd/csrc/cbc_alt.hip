/*
 * cbc_alt.hip -- ARIA-CBC and Camellia-CBC + HMAC record protection for TLS 1.2
 * / DTLS 1.2: the record kernel of tlsrec_cbc_kernel.h (see cbc.hip) around the
 * S-box image ciphers of tlsrec_device.h, and the key setup of their slots.
 * A unit of its own, as gcm_alt_*.hip are, so that the parallel build is no
 * longer than its longest unit.
 *
 * The four (cipher, MAC) pairs of the reference's suites (ssl_ciphersuites.c),
 * both directions each:
 *     NR 12  ARIA-128      HMAC-SHA256        NR 18  Camellia-128  HMAC-SHA256
 *     NR 16  ARIA-256      HMAC-SHA384        NR 24  Camellia-256  HMAC-SHA384
 *
 * Both ciphers decrypt with their forward function under a derived key array
 * (RFC 5794 2.2, RFC 3713 2.3; tlsrec_altkey.h), so the kernels hold one block
 * function.  A slot keeps the encryption keys in SlotState::ark, exactly as an
 * ARIA- / Camellia-GCM slot does, and the decryption keys in the same word
 * layout at the start of SlotState::rk / rkr, which a slot without AES keys
 * does not otherwise use.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tlsrec.h"
#include "tlsrec_altkey.h"
#include "tlsrec_cbc.h"
#include "tlsrec_cbc_kernel.h"
#include "tlsrec_device.h"
#include "tlsrec_internal.h"

namespace tlsrec {

/* Key setup of ARIA-CBC / Camellia-CBC slots: one workgroup per slot, as
 * tlsrec_cbc_keysetup_kernel; lane 0 expands the key (the cipher's S-boxes
 * staged in LDS, as the AEAD key setup stages them), derives the decryption
 * keys and the HMAC midstates, the workgroup stores them.  Every word of rk,
 * rkr and ark, h, hpow and the slot's whole table area is written, so nothing
 * of an earlier owner -- AEAD, AES-CBC or another key of these ciphers --
 * survives.  The engine hands it runs of ARIA / Camellia material only (AES:
 * tlsrec_cbc_keysetup_kernel); the guard below is for safety alone. */
__global__ __launch_bounds__(64) void tlsrec_cbc_alt_keysetup_kernel(SlotState *slots, uint4 *ghtab, uint8_t *cipher_of,
                                                                     const tlsrec_cbc_key_material *keys,
                                                                     uint32_t first, uint32_t count)
{
    __shared__ uint8_t sb[4 * 256];
    __shared__ uint64_t ksched[34];           /* 17 ARIA round keys as bytes, or 34 Camellia subkeys */
    __shared__ uint32_t ek[ALT_KEY_WORDS], dk[ALT_KEY_WORDS], ms[CBC_MS_WORDS];
    if (blockIdx.x >= count) return;
    const uint32_t slot = first + blockIdx.x;
    const tlsrec_cbc_key_material *k = &keys[blockIdx.x];
    SlotState *st = &slots[slot];
    const int tid = threadIdx.x;
    const int cipher = k->cipher, mac = k->mac;
    if (!cbc_is_alt(cipher)) return;          /* uniform, before the barriers */
    const bool cam = cipher >= TLSREC_CIPHER_CAMELLIA_128_CBC;
    const int keylen = (int) cbc_keylen(cipher);
    for (int i = tid; i < 4 * 256; i += 64) sb[i] = cam ? kCamSbox.v[i >> 8][i & 255] : kAriaSbox.v[i >> 8][i & 255];
    __syncthreads();
    if (tid == 0) {
        int nr;
        if (cam) {
            nr = cam_key_expand(sb, k->key, keylen, ksched);
            for (int i = 0; i < 34; i++) {
                ek[2 * i] = (uint32_t) (ksched[i] >> 32);
                ek[2 * i + 1] = (uint32_t) ksched[i];
            }
            cam_dec_keys(ek, nr, dk);
        } else {
            uint8_t (*eb)[16] = reinterpret_cast<uint8_t (*)[16]>(ksched);
            nr = aria_key_expand(sb, k->key, keylen, eb);
            for (int e = 0; e < 17; e++)
                for (int c = 0; c < 4; c++)
                    ek[4 * e + c] = e <= nr ? ((uint32_t) eb[e][4 * c] | ((uint32_t) eb[e][4 * c + 1] << 8) |
                                               ((uint32_t) eb[e][4 * c + 2] << 16) | ((uint32_t) eb[e][4 * c + 3] << 24))
                                            : 0u;
            aria_dec_keys(ek, nr, dk);
        }
        if (mac == TLSREC_MAC_SHA256) cbc_hmac_midstates<TLSREC_MAC_SHA256>(k->mac_key, ms);
        else cbc_hmac_midstates<TLSREC_MAC_SHA384>(k->mac_key, ms);
        tlsrec_key_material km;
        __builtin_memset(&km, 0, sizeof(km));
        km.cipher = (uint8_t) cipher;
        km.tls_minor = 3;
        km.reserved[1] = (uint8_t) mac;       /* [0] mirrors the CID length (tlsrec_keytab_set_cid) */
        km.reserved[2] = k->etm;
        st->km = km;
        for (int i = 0; i < keylen; i++) st->km.key[i] = k->key[i];
        st->nr = (uint32_t) nr;
        st->cid_len = 0;                      /* a (re)load leaves the slot without a CID */
        for (int i = 0; i < 16; i++) {
            st->h[i] = 0;
            st->hpow[i >> 2][i & 3] = 0;
        }
        cipher_of[slot] = (uint8_t) cipher;
    }
    __syncthreads();
    for (int i = tid; i < 120; i += 64) {
        const uint32_t d = i < ALT_KEY_WORDS ? dk[i] : 0u;    /* the decryption keys, then zeros to the end of rkr */
        if (i < 60) st->rk[i] = d;
        else st->rkr[i - 60] = d;
        if (i < ALT_KEY_WORDS) st->ark[i] = ek[i];
    }
    uint32_t *mw = reinterpret_cast<uint32_t *>(ghtab + (size_t) slot * KEY_TABLE_WORDS);
    if (tid < CBC_MS_WORDS) mw[tid] = ms[tid];
    uint4 *tab = ghtab + (size_t) slot * KEY_TABLE_WORDS;
    for (int i = CBC_MS_WORDS / 4 + tid; i < KEY_TABLE_WORDS; i += 64) tab[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (tid < CBC_MS_WORDS) ms[tid] = 0;     /* key-derived values out of LDS */
    if (tid < 34) ksched[tid] = 0;
    for (int i = tid; i < ALT_KEY_WORDS; i += 64) {
        ek[i] = 0;
        dk[i] = 0;
    }
}

} /* namespace tlsrec */

using namespace tlsrec;

extern "C" hipError_t tlsrec__launch_cbc_alt_keysetup(SlotState *slots, uint4 *ghtab, uint8_t *cipher_of,
                                                      const tlsrec_cbc_key_material *keys, uint32_t first,
                                                      uint32_t count, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(tlsrec_cbc_alt_keysetup_kernel, dim3(count), dim3(64), 0, st, slots, ghtab, cipher_of, keys,
                       first, count);
    return hipGetLastError();
}

/* variants, grid: as tlsrec__launch_cbc (cbc.hip), which hands its own on */
extern "C" hipError_t tlsrec__launch_cbc_alt(const CbcArgs *a, int dec, uint32_t variants, uint32_t grid, hipStream_t st)
{
    hipError_t e = hipSuccess;
#define TLSREC_CBC_LAUNCH(NR, CIPHER, MAC)                                                                          \
    if (e == hipSuccess && (variants & cbc_variant_bit(CIPHER, MAC))) {                                             \
        if (dec) hipLaunchKernelGGL((tlsrec_cbc_kernel<NR, MAC, true>), dim3(grid), dim3(CBC_THREADS), 0, st, *a);  \
        else hipLaunchKernelGGL((tlsrec_cbc_kernel<NR, MAC, false>), dim3(grid), dim3(CBC_THREADS), 0, st, *a);     \
        e = hipGetLastError();                                                                                      \
    }
    TLSREC_CBC_LAUNCH(12, TLSREC_CIPHER_ARIA_128_CBC, TLSREC_MAC_SHA256)
    TLSREC_CBC_LAUNCH(16, TLSREC_CIPHER_ARIA_256_CBC, TLSREC_MAC_SHA384)
    TLSREC_CBC_LAUNCH(18, TLSREC_CIPHER_CAMELLIA_128_CBC, TLSREC_MAC_SHA256)
    TLSREC_CBC_LAUNCH(24, TLSREC_CIPHER_CAMELLIA_256_CBC, TLSREC_MAC_SHA384)
#undef TLSREC_CBC_LAUNCH
    return e;
}
