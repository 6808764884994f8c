/*
 * cbc.hip -- AES-CBC + HMAC record protection for TLS 1.2 / DTLS 1.2: the
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
#include "tlsrec_device.h"
#include "tlsrec_frame.h"
#include "tlsrec_internal.h"
#include "tlsrec_recdev.h"

namespace tlsrec {

constexpr int CBC_WAVES = 8;
constexpr int CBC_THREADS = CBC_WAVES * 64;

/* the digest (big-endian words) as bytes at p */
template <int N>
__device__ __forceinline__ void put_digest(uint8_t *p, const uint32_t (&dig)[N])
{
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint32_t w = cbc_bswap(dig[i]);
        __builtin_memcpy(p + 4 * i, &w, 4);
    }
}

/* digest byte at a run-time index below 4 N, by selects over the words */
template <int N>
__device__ __forceinline__ uint32_t digest_byte(const uint32_t (&dig)[N], uint32_t idx)
{
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < N; i++) w = (idx >> 2) == (uint32_t) i ? dig[i] : w;
    return (w >> (24 - 8 * (idx & 3))) & 0xff;
}

template <int NR, int MAC, bool DEC>
__global__ __launch_bounds__(CBC_THREADS) void tlsrec_cbc_kernel(CbcArgs a)
{
    using H = CbcHash<MAC>;
    constexpr uint32_t ML = 4 * H::DIGW;                       /* maclen */
    __shared__ __attribute__((aligned(16))) uint8_t lds[65536];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t lanebase = (uint32_t) (lane & 31) << 2;
    const uint32_t lo = a.perm ? *a.lo : 0u;
    const uint32_t count = a.perm ? *a.hi - lo : (uint32_t) a.n;
    const uint64_t wg_base = (uint64_t) blockIdx.x * CBC_THREADS;
    if (wg_base >= count) return;                              /* uniform, before the barrier */
    if constexpr (DEC)
        cbc_fill_dec_tables(lds, tid, CBC_THREADS);
    else
        aes_fill_tables(lds, tid, CBC_THREADS);
    __syncthreads();

    uint32_t my_slot = 0xffffffffu, my_rec = 0;
    {
        const uint64_t pos = wg_base + (uint64_t) tid;
        if (pos < count) {
            my_rec = a.perm ? a.perm[lo + pos] : (uint32_t) pos;
            const uint32_t s = a.recs[my_rec].slot;
            const bool usable = s < a.capacity && a.slots[s].km.cipher != 0;
            const int c = usable ? a.slots[s].km.cipher : 0;   /* no read past the table */
            if (TLSREC_HOOK_SKIP(my_rec, a.skip)) {
                /* test hook: an unreached record keeps the guard's INTERNAL_ERROR */
            } else if (usable && cbc_is_cipher(c) && cbc_keylen(c) / 4 + 6 == NR && a.slots[s].km.reserved[1] == MAC)
                my_slot = s;
            else if (!a.perm && !usable)
                bad_slot_result(a.recs[my_rec], &a.res[my_rec]);   /* identity order */
        }
    }

    for (;;) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(wave_min(my_slot));
        if (s == 0xffffffffu) break;
        const bool mine = my_slot == s;
        my_slot = mine ? 0xffffffffu : my_slot;
        if (!mine) continue;
        const SlotState *sl = &a.slots[s];
        const kconst_u32 *rk = (const kconst_u32 *) (uintptr_t) (DEC ? sl->ark : sl->rkr);
        const kconst_u32 *ms = (const kconst_u32 *) (uintptr_t) (a.ghtab + (size_t) s * KEY_TABLE_WORDS);
        const uint32_t etm = sl->km.reserved[2], cidl = sl->km.reserved[0];
        const tlsrec_batch_rec *dp = &a.recs[my_rec];
        const tlsrec_batch_rec d = *dp;

        CbcAad A;
        A.ctr = dp->ctr;
        A.cid = sl->cid;
        A.cid_len = cidl;
        A.type = d.type;
        A.ver0 = d.ver[0];
        A.ver1 = d.ver[1];
        A.len_field = 0;
        A.aad_len = cidl ? 23 + cidl : 13;

        tlsrec_batch_res r;
        r.cid_len = 0;
        r.reserved[0] = r.reserved[1] = 0;
        uint32_t off = d.data_offset, len = d.data_len, type = d.type;
        int32_t status = 0;
        uint32_t dig[H::DIGW];

        if constexpr (!DEC) {
            uint32_t ilen = 0, plen = 0, padlen = 0;
            const uint32_t clen = len;
            if (d.buf_len < off || d.buf_len - off < len) {                        /* ssl_msg.c:814-823 */
                status = TLSREC_E_INTERNAL_ERROR;
            } else if (len > TLSREC_OUT_CONTENT_LEN) {                             /* :833-839 */
                status = TLSREC_E_BAD_INPUT_DATA;
            } else {
                uint32_t post = d.buf_len - (len + off);
                r.cid_len = (uint8_t) cidl;                                        /* :874 */
                if (cidl) {                                                        /* DTLSInnerPlaintext, :878-898 */
                    const uint32_t pad = (0u - (len + 1)) & (TLSREC_PADDING_GRANULARITY - 1);
                    if (post == 0 || post - 1 < pad) {
                        status = TLSREC_E_BUFFER_TOO_SMALL;
                    } else {
                        len += 1 + pad;
                        type = TLSREC_MSG_CID;
                        post = d.buf_len - (len + off);
                    }
                }
                ilen = len;
                if (!status && !etm) {                                             /* :909 */
                    if (post < ML) status = TLSREC_E_BUFFER_TOO_SMALL;
                    else { len += ML; post -= ML; }
                }
                if (!status) {
                    padlen = 15u - (len & 15u);                                    /* :1092-1095 */
                    if (post < padlen + 1) status = TLSREC_E_BUFFER_TOO_SMALL;     /* :1098 */
                    else { len += padlen + 1; post -= padlen + 1; }
                }
                if (!status && off < 16) status = TLSREC_E_BUFFER_TOO_SMALL;       /* :1116 */
                if (!status) {
                    plen = len;
                    off -= 16;                                                     /* :1186-1188 */
                    len += 16;
                    if (etm && post < ML) status = TLSREC_E_BUFFER_TOO_SMALL;      /* :1199 */
                }
            }
            if (!status) {
                const uint8_t *src = a.in + d.buf_off + d.data_offset;
                uint8_t *dst = a.out + d.buf_off + d.data_offset;
                /* the (inner) plaintext in the output buffer */
                if (src != dst || cidl) {
                    for (uint32_t pos = 0; pos < ilen; pos += 16) {
                        const uint4 v = load_block(src, pos, clen, ilen, d.type, pos + 16 <= clen);
                        store_block(dst, pos, ilen, v, true);
                    }
                }
                A.type = type;
#pragma unroll 1
                for (uint32_t ph = 0; ph < 2; ph++) {
                    if ((ph == 0) == (etm == 0)) {
                        /* MAC over the plaintext, or over IV || ciphertext (:1196) */
                        const uint32_t hl = etm ? 16 + plen : ilen;
                        A.len_field = hl;
                        cbc_hmac<MAC>(dig, ms, A, etm ? dst - 16 : dst, hl, hl, hl);
                        put_digest(dst + (etm ? plen : ilen), dig);
                    } else {
                        const uint32_t body = plen - padlen - 1;                   /* content (+ MAC) */
                        for (uint32_t i = 0; i <= padlen; i++) dst[body + i] = (uint8_t) padlen;   /* :1103-1105 */
                        uint4 x = cbc_ld16(src - 16);                              /* the caller's IV */
                        gstore16(dst - 16, x);
                        for (uint32_t pos = 0; pos < plen; pos += 16) {
                            x = aes_encrypt<NR, 0>(lds, lanebase, rk, xor4(x, gload16(dst + pos)));
                            gstore16(dst + pos, x);
                        }
                    }
                }
                if (etm) len += ML;
            }
        } else {
            uint32_t clen = 0, padlen = 0, correct = 0;
            if (d.buf_len < off || d.buf_len - off < len) {                        /* :1302-1308 */
                status = TLSREC_E_INTERNAL_ERROR;
            } else {
                bool cid_ok = d.cid_len == cidl;                                   /* :1317-1320 */
                if (cid_ok && cidl) {
                    const uint32_t co = (uint32_t) d.cid_off[0] | ((uint32_t) d.cid_off[1] << 8) |
                                        ((uint32_t) d.cid_off[2] << 16) | ((uint32_t) d.cid_off[3] << 24);
                    const uint8_t *rc = a.in + d.buf_off + co;
                    for (uint32_t i = 0; i < cidl; i++) cid_ok = cid_ok && rc[i] == sl->cid[i];
                }
                if (!cid_ok) {
                    status = TLSREC_E_UNEXPECTED_CID;
                } else if (len < 32 || len < 16 + ML + 1) {                        /* :1472-1482 */
                    status = TLSREC_E_INVALID_MAC;
                } else {
                    if (etm) len -= ML;                                            /* :1503 */
                    if (len & 15u) status = TLSREC_E_INVALID_MAC;                  /* :1557-1562 (same result before the MAC) */
                }
            }
            if (!status) {
                const uint8_t *src = a.in + d.buf_off + d.data_offset;             /* the IV */
                uint8_t *pdst = a.out + d.buf_off + d.data_offset + 16;            /* the plaintext */
                clen = len - 16;
#pragma unroll 1
                for (uint32_t ph = 0; ph < 2 && !status; ph++) {
                    if ((ph == 0) == (etm != 0)) {
                        /* encrypt-then-MAC: over IV || ciphertext, all public; MAC-then-encrypt:
                         * over the plaintext, content length secret (constant flow, file head) */
                        const uint32_t maxL = etm ? len : clen - ML;
                        const uint32_t L = etm ? len : len - ML;
                        A.len_field = L;
                        cbc_hmac<MAC>(dig, ms, A, etm ? src : pdst, L, maxL, etm ? len : clen);
                        uint32_t diff = 0;
                        if (etm) {
#pragma unroll
                            for (int i = 0; i < H::DIGW; i++) diff |= ld_u32le(src + len + 4 * i) ^ cbc_bswap(dig[i]);
                        } else {
                            len = L;                                               /* :1738 */
                            const uint32_t minL = maxL > 256 ? maxL - 256 : 0;
                            for (uint32_t j = minL; j < clen; j++) {               /* mbedtls_ct_memcpy_offset + ct_memcmp */
                                const uint32_t idx = j - L;
                                const uint32_t x = (uint32_t) pdst[j] ^ digest_byte(dig, idx < ML ? idx : 0u);
                                diff |= idx < ML ? x : 0u;
                            }
                            diff |= correct ^ 1u;
                        }
                        status = diff ? TLSREC_E_INVALID_MAC : 0;
                    } else {
                        uint4 prev = cbc_ld16(src), p = make_uint4(0, 0, 0, 0);
                        for (uint32_t pos = 0; pos < clen; pos += 16) {
                            const uint4 c = gload16(src + 16 + pos);
                            p = xor4(cbc_aes_decrypt<NR>(lds, lanebase, rk, c), prev);
                            prev = c;
                            gstore16(pdst + pos, p);
                        }
                        off += 16;                                                 /* :1572-1573 */
                        len = clen;
                        padlen = p.w >> 24;                                        /* :1627 */
                        const uint32_t ge = etm ? (len >= padlen + 1) : (len >= ML + padlen + 1);   /* :1629-1651 */
                        correct = ge;
                        padlen = (ge ? padlen : 0u) + 1;
                        const uint32_t padding_idx = len - padlen;
                        const uint32_t num_checks = len <= 256 ? len : 256;
                        uint32_t pad_count = 0;
                        for (uint32_t idx = len - num_checks; idx < len; idx++)    /* :1675-1684 */
                            pad_count += (uint32_t) (idx >= padding_idx) & (uint32_t) (pdst[idx] == padlen - 1);
                        correct &= (uint32_t) (pad_count == padlen);
                        padlen = correct ? padlen : 0u;
                        len -= padlen;                                             /* :1700 */
                        if (etm) status = correct ? 0 : TLSREC_E_INVALID_MAC;
                    }
                }
                if (!status && cidl) {                                             /* ssl_parse_inner_plaintext, :1822-1828 */
                    uint32_t n = len;
                    while (n > 0 && pdst[n - 1] == 0) n--;
                    if (n == 0) {
                        status = TLSREC_E_INVALID_RECORD;
                    } else {
                        type = pdst[n - 1];
                        len = n - 1;
                    }
                }
            }
        }
        r.status = status;
        r.data_offset = off;
        r.data_len = len;
        r.type = (uint8_t) type;
        a.res[my_rec] = r;
    }
}

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
 * key setup does not overwrite: the decryption round keys (SlotState::ark)
 * and the HMAC midstates.  One workgroup per slot; slots of other ciphers are
 * left alone.  Runs before the slots' cipher_of entries change. */
__global__ __launch_bounds__(64) void tlsrec_cbc_wipe_kernel(SlotState *slots, uint4 *ghtab, const uint8_t *cipher_of,
                                                             uint32_t first, uint32_t count)
{
    if (blockIdx.x >= count) return;
    const uint32_t slot = first + blockIdx.x;
    if (!cbc_is_cipher(cipher_of[slot])) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < 68; i += 64) slots[slot].ark[i] = 0;
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
    const int nk = (int) cbc_keylen(cipher) / 4, nr = nk + 6;
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

extern "C" hipError_t tlsrec__launch_cbc_keysetup(SlotState *slots, uint4 *ghtab, uint8_t *cipher_of,
                                                  const tlsrec_cbc_key_material *keys, uint32_t first, uint32_t count,
                                                  hipStream_t st)
{
    if (count == 0) return hipSuccess;
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
    return e;
}
