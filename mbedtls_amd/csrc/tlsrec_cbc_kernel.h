/*
 * tlsrec_cbc_kernel.h -- the CBC + HMAC record kernel (see cbc.hip for its
 * shape and the constant flow of MAC-then-encrypt decryption), a template so
 * that its instantiations spread over compile units: cbc.hip holds the AES
 * ones, cbc_alt.hip the ARIA and Camellia ones.
 *
 * NR picks the block cipher as it does in blk_encrypt (tlsrec_device.h):
 * 10 / 14 AES on the T / Td tables (64 KiB of LDS), 12 / 16 ARIA and 18 / 24
 * Camellia on the S-box image (32 KiB).  ARIA and Camellia decrypt with their
 * forward function under the slot's decryption key array (tlsrec_altkey.h), so
 * for them both directions run blk_encrypt; everything around the block
 * function is one code for every cipher.
 */
#ifndef TLSREC_CBC_KERNEL_H
#define TLSREC_CBC_KERNEL_H

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

/* The additional data of a record under slot sl (len_field is set by the caller per MAC) */
__device__ __forceinline__ CbcAad cbc_record_aad(const tlsrec_batch_rec *dp, const SlotState *sl, uint32_t cidl)
{
    CbcAad A;
    A.ctr = dp->ctr;
    A.cid = sl->cid;
    A.cid_len = cidl;
    A.type = dp->type;
    A.ver0 = dp->ver[0];
    A.ver1 = dp->ver[1];
    A.len_field = 0;
    A.aad_len = cidl ? 23 + cidl : 13;
    return A;
}

/* Decryption, the checks before a record byte is used (ssl_msg.c:1302-1320,
 * :1472-1482, :1503, :1557-1562).  len: data_len on entry; with status 0 the
 * length of IV || ciphertext (the encrypt-then-MAC tag taken off). */
__device__ __forceinline__ int32_t cbc_dec_frame(const tlsrec_batch_rec &d, const SlotState *sl, const uint8_t *in,
                                                 uint32_t cidl, uint32_t etm, uint32_t ML, uint32_t &len)
{
    if (d.buf_len < d.data_offset || d.buf_len - d.data_offset < len)          /* :1302-1308 */
        return TLSREC_E_INTERNAL_ERROR;
    bool cid_ok = d.cid_len == cidl;                                           /* :1317-1320 */
    if (cid_ok && cidl) {
        const uint32_t co = (uint32_t) d.cid_off[0] | ((uint32_t) d.cid_off[1] << 8) |
                            ((uint32_t) d.cid_off[2] << 16) | ((uint32_t) d.cid_off[3] << 24);
        const uint8_t *rc = in + d.buf_off + co;
        for (uint32_t i = 0; i < cidl; i++) cid_ok = cid_ok && rc[i] == sl->cid[i];
    }
    if (!cid_ok) return TLSREC_E_UNEXPECTED_CID;
    if (len < 32 || len < 16 + ML + 1) return TLSREC_E_INVALID_MAC;            /* :1472-1482 */
    if (etm) len -= ML;                                                        /* :1503 */
    return (len & 15u) ? TLSREC_E_INVALID_MAC : 0;                             /* :1557-1562 (same result before the MAC) */
}

/* The padding check of ssl_msg.c:1627-1700 over the plaintext pdst[0, len),
 * last = its last byte: min(256, len) byte loads, the count of matching bytes
 * a sum of compares.  Returns len less the padding (less nothing when it is
 * wrong); correct: 1 / 0. */
__device__ __forceinline__ uint32_t cbc_check_padding(const uint8_t *pdst, uint32_t len, uint32_t last, uint32_t ML,
                                                      uint32_t etm, uint32_t &correct)
{
    uint32_t padlen = last;                                                    /* :1627 */
    const uint32_t ge = etm ? (len >= padlen + 1) : (len >= ML + padlen + 1);  /* :1629-1651 */
    correct = ge;
    padlen = (ge ? padlen : 0u) + 1;
    const uint32_t padding_idx = len - padlen;
    const uint32_t num_checks = len <= 256 ? len : 256;
    uint32_t pad_count = 0;
    for (uint32_t idx = len - num_checks; idx < len; idx++)                    /* :1675-1684 */
        pad_count += (uint32_t) (idx >= padding_idx) & (uint32_t) (pdst[idx] == padlen - 1);
    correct &= (uint32_t) (pad_count == padlen);
    padlen = correct ? padlen : 0u;
    return len - padlen;                                                       /* :1700 */
}

/* MAC-then-encrypt: the peer's MAC at pdst[L, L + maclen) against dig, L secret
 * (mbedtls_ct_memcpy_offset + mbedtls_ct_memcmp): maclen + min(256, maxL) byte
 * loads over [maxL - min(256, maxL), clen); non-zero = they differ */
template <int N>
__device__ __forceinline__ uint32_t cbc_peer_mac_diff(const uint8_t *pdst, const uint32_t (&dig)[N], uint32_t L,
                                                      uint32_t maxL, uint32_t clen)
{
    constexpr uint32_t ML = 4 * N;
    uint32_t diff = 0;
    const uint32_t minL = maxL > 256 ? maxL - 256 : 0;
    for (uint32_t j = minL; j < clen; j++) {
        const uint32_t idx = j - L;
        const uint32_t x = (uint32_t) pdst[j] ^ digest_byte(dig, idx < ML ? idx : 0u);
        diff |= idx < ML ? x : 0u;
    }
    return diff;
}

/* ssl_parse_inner_plaintext (:1822-1828) of a record with a connection ID */
__device__ __forceinline__ int32_t cbc_inner_plaintext(const uint8_t *pdst, uint32_t &len, uint32_t &type)
{
    uint32_t n = len;
    while (n > 0 && pdst[n - 1] == 0) n--;
    if (n == 0) return TLSREC_E_INVALID_RECORD;
    type = pdst[n - 1];
    len = n - 1;
    return 0;
}

template <int NR, int MAC, bool DEC>
__global__ __launch_bounds__(CBC_THREADS) void tlsrec_cbc_kernel(CbcArgs a)
{
    using H = CbcHash<MAC>;
    constexpr uint32_t ML = 4 * H::DIGW;                       /* maclen */
    constexpr bool ALT = NR != 10 && NR != 14;                 /* ARIA / Camellia: the S-box image */
    __shared__ __attribute__((aligned(16))) uint8_t lds[ALT ? 32768 : 65536];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t lanebase = (uint32_t) (lane & 31) << 2;
    const uint32_t lo = a.perm ? *a.lo : 0u;
    const uint32_t count = a.perm ? *a.hi - lo : (uint32_t) a.n;
    const uint64_t wg_base = (uint64_t) blockIdx.x * CBC_THREADS;
    if (wg_base >= count) return;                              /* uniform, before the barrier */
    if constexpr (ALT)
        alt_fill_tables<NR>(lds, tid, CBC_THREADS);
    else if constexpr (DEC)
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
            } else if (usable && (ALT ? cbc_nr(c) == NR
                                      : c >= TLSREC_CIPHER_AES_128_CBC && c <= TLSREC_CIPHER_AES_256_CBC &&
                                            cbc_aes_keylen(c) / 4 + 6 == NR) &&
                       a.slots[s].km.reserved[1] == MAC)
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
        /* AES: rkr encrypts, ark decrypts; ARIA / Camellia: ark encrypts, the key array in rk / rkr decrypts */
        const kconst_u32 *rk = (const kconst_u32 *) (uintptr_t) (ALT ? (DEC ? sl->rk : sl->ark) : (DEC ? sl->ark : sl->rkr));
        const kconst_u32 *ms = (const kconst_u32 *) (uintptr_t) (a.ghtab + (size_t) s * KEY_TABLE_WORDS);
        const uint32_t etm = sl->km.reserved[2], cidl = sl->km.reserved[0];
        const tlsrec_batch_rec *dp = &a.recs[my_rec];
        const tlsrec_batch_rec d = *dp;

        CbcAad A = cbc_record_aad(dp, sl, cidl);

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
                            x = blk_encrypt<NR, ALT>(lds, lanebase, rk, xor4(x, gload16(dst + pos)));
                            gstore16(dst + pos, x);
                        }
                    }
                }
                if (etm) len += ML;
            }
        } else {
            uint32_t clen = 0, correct = 0;
            status = cbc_dec_frame(d, sl, a.in, cidl, etm, ML, len);
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
                            diff = cbc_peer_mac_diff(pdst, dig, L, maxL, clen);
                            diff |= correct ^ 1u;
                        }
                        status = diff ? TLSREC_E_INVALID_MAC : 0;
                    } else {
                        uint4 prev = cbc_ld16(src), p = make_uint4(0, 0, 0, 0);
                        for (uint32_t pos = 0; pos < clen; pos += 16) {
                            const uint4 c = gload16(src + 16 + pos);
                            if constexpr (ALT)
                                p = xor4(blk_encrypt<NR, true>(lds, lanebase, rk, c), prev);
                            else
                                p = xor4(cbc_aes_decrypt<NR>(lds, lanebase, rk, c), prev);
                            prev = c;
                            gstore16(pdst + pos, p);
                        }
                        off += 16;                                                 /* :1572-1573 */
                        len = cbc_check_padding(pdst, clen, p.w >> 24, ML, etm, correct);
                        if (etm) status = correct ? 0 : TLSREC_E_INVALID_MAC;
                    }
                }
                if (!status && cidl) status = cbc_inner_plaintext(pdst, len, type);
            }
        }
        r.status = status;
        r.data_offset = off;
        r.data_len = len;
        r.type = (uint8_t) type;
        a.res[my_rec] = r;
    }
}

} /* namespace tlsrec */

#endif /* TLSREC_CBC_KERNEL_H */
