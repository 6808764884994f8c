/*
 * tlsrec_cbc_wave.h -- CBC + HMAC decryption with a wave per record, for the
 * coalesced single-record path (engine.hip run_batch): a few records, each
 * alone under its key, where the lane kernel of tlsrec_cbc_kernel.h would run
 * a whole record on one lane of an otherwise idle workgroup.
 *
 * CBC decryption has no chain: plaintext block i is D(c[i]) ^ c[i - 1].  So
 * the 64 lanes of a wave decrypt 64 blocks of ONE record per round, lane q
 * the blocks q, q + 64, ...; the hash stays one dependent chain and runs on
 * lane 0 with the other lanes idle.  Everything but the cipher loop is the
 * lane kernel's own code (cbc_dec_frame, cbc_hmac, cbc_check_padding,
 * cbc_peer_mac_diff, cbc_inner_plaintext), with the same order of phases, the
 * same statuses and the same constant flow of MAC-then-encrypt decryption
 * (cbc.hip, file head): every trip count and address below is fixed by the
 * record's public lengths.
 *
 * In place (in == out, as the coalesced path always runs) plaintext block i
 * lands on ciphertext block i, which is lane q + 1's `prev`.  No lane reads a
 * `prev` from memory: within a round it comes from the neighbouring lane's
 * registers, which were loaded before any lane of the wave stores (one
 * instruction stream), and across rounds lane 0 takes lane 63's ciphertext
 * block of the round before from a register carried through v_readlane.
 *
 * After the cipher loop lane 0 reads plaintext that other lanes of its wave
 * stored.  A workgroup-scope fence stands between the two: on gfx950 it is the
 * wave's s_waitcnt vmcnt(0) and no cache operation -- a CU's vector L1 is
 * write-through and coherent with that CU's own stores -- and it keeps the
 * compiler from moving the loads above the stores.
 *
 * Identity order only (CbcArgs::perm is not read): record r belongs to wave
 * r % CBC_WAVE_WAVES of workgroup r / CBC_WAVE_WAVES.  The workgroup is as
 * large as the lane kernel's, 8 waves: the table fill (64 KiB of Td tables, or
 * the 32 KiB S-box image) is the fixed cost of a launch and 512 threads write
 * it in two (one) steps of four 16-byte stores each, while a batch of one
 * record, the common case, gains nothing from fewer waves.
 */
#ifndef TLSREC_CBC_WAVE_H
#define TLSREC_CBC_WAVE_H

#include "tlsrec_cbc_kernel.h"

namespace tlsrec {

constexpr int CBC_WAVE_WAVES = 8;
constexpr int CBC_WAVE_THREADS = CBC_WAVE_WAVES * 64;

/* lane q: lane q - 1's v (lane 0: its own) */
__device__ __forceinline__ uint4 cbc_wave_up1(uint4 v)
{
    return make_uint4(__shfl_up(v.x, 1), __shfl_up(v.y, 1), __shfl_up(v.z, 1), __shfl_up(v.w, 1));
}

/* every lane: lane 63's v */
__device__ __forceinline__ uint4 cbc_wave_last(uint4 v)
{
    return make_uint4(__builtin_amdgcn_readlane(v.x, 63), __builtin_amdgcn_readlane(v.y, 63),
                      __builtin_amdgcn_readlane(v.z, 63), __builtin_amdgcn_readlane(v.w, 63));
}

template <int NR, int MAC>
__global__ __launch_bounds__(CBC_WAVE_THREADS) void tlsrec_cbc_wave_kernel(CbcArgs a)
{
    using H = CbcHash<MAC>;
    constexpr uint32_t ML = 4 * H::DIGW;                       /* maclen */
    constexpr bool ALT = NR != 10 && NR != 14;                 /* ARIA / Camellia: the S-box image */
    __shared__ __attribute__((aligned(16))) uint8_t lds[ALT ? 32768 : 65536];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t lanebase = (uint32_t) (lane & 31) << 2;
    if ((uint64_t) blockIdx.x * CBC_WAVE_WAVES >= a.n) return; /* uniform, before the barrier */
    if constexpr (ALT)
        alt_fill_tables<NR>(lds, tid, CBC_WAVE_THREADS);
    else
        cbc_fill_dec_tables(lds, tid, CBC_WAVE_THREADS);
    __syncthreads();

    /* from here on every branch but `lane == 0` is wave-uniform */
    const uint32_t rec = __builtin_amdgcn_readfirstlane(blockIdx.x * CBC_WAVE_WAVES + ((uint32_t) tid >> 6));
    if (rec >= a.n) return;
    if (TLSREC_HOOK_SKIP(rec, a.skip)) return;                 /* test hook: keeps the guard's INTERNAL_ERROR */
    const tlsrec_batch_rec *dp = &a.recs[rec];
    const tlsrec_batch_rec d = *dp;
    const uint32_t s = d.slot;
    const bool usable = s < a.capacity && a.slots[s].km.cipher != 0;
    if (!usable) {
        if (lane == 0) bad_slot_result(d, &a.res[rec]);
        return;
    }
    const SlotState *sl = &a.slots[s];
    const int c = sl->km.cipher;
    if (!((ALT ? cbc_nr(c) == NR
               : c >= TLSREC_CIPHER_AES_128_CBC && c <= TLSREC_CIPHER_AES_256_CBC && cbc_aes_keylen(c) / 4 + 6 == NR) &&
          sl->km.reserved[1] == MAC))
        return;                                                /* another launch's record */
    /* AES: ark decrypts; ARIA / Camellia: the key array in rk / rkr decrypts */
    const kconst_u32 *rk = (const kconst_u32 *) (uintptr_t) (ALT ? sl->rk : sl->ark);
    const kconst_u32 *ms = (const kconst_u32 *) (uintptr_t) (a.ghtab + (size_t) s * KEY_TABLE_WORDS);
    const uint32_t etm = sl->km.reserved[2], cidl = sl->km.reserved[0];

    CbcAad A = cbc_record_aad(dp, sl, cidl);
    uint32_t off = d.data_offset, len = d.data_len, type = d.type;
    int32_t status = cbc_dec_frame(d, sl, a.in, cidl, etm, ML, len);
    if (!status) {
        const uint8_t *src = a.in + d.buf_off + d.data_offset;                     /* the IV */
        uint8_t *pdst = a.out + d.buf_off + d.data_offset + 16;                    /* the plaintext */
        const uint32_t clen = len - 16;
        uint32_t correct = 0;                                                      /* lane 0's */
#pragma unroll 1
        for (uint32_t ph = 0; ph < 2 && !status; ph++) {
            if ((ph == 0) == (etm != 0)) {
                /* the hash, one chain: lane 0.  Encrypt-then-MAC: over IV || ciphertext, all public, and
                 * before a byte is written; MAC-then-encrypt: over the plaintext, content length secret */
                if (lane == 0) {
                    const uint32_t maxL = etm ? len : clen - ML;
                    const uint32_t L = etm ? len : len - ML;
                    uint32_t dig[H::DIGW];
                    A.len_field = L;
                    cbc_hmac<MAC>(dig, ms, A, etm ? src : pdst, L, maxL, etm ? len : clen);
                    uint32_t diff = 0;
                    if (etm) {
#pragma unroll
                        for (int i = 0; i < H::DIGW; i++) diff |= ld_u32le(src + len + 4 * i) ^ cbc_bswap(dig[i]);
                    } else {
                        len = L;                                                   /* :1738 */
                        diff = cbc_peer_mac_diff(pdst, dig, L, maxL, clen);
                        diff |= correct ^ 1u;
                    }
                    status = diff ? TLSREC_E_INVALID_MAC : 0;
                }
            } else {
                /* the cipher: clen / 16 blocks, 64 a round.  `carry` is the block before the round's
                 * first: the IV, then lane 63's ciphertext block of the round before. */
                const uint32_t nblk = clen >> 4;
                uint4 carry = cbc_ld16(src);
#pragma unroll 1
                for (uint32_t base = 0; base < nblk; base += 64) {
                    const uint32_t i = base + (uint32_t) lane;
                    const bool live = i < nblk;
                    uint4 cb = make_uint4(0, 0, 0, 0);
                    if (live) cb = gload16(src + 16 + 16 * (size_t) i);
                    const uint4 up = cbc_wave_up1(cb);
                    const uint4 prev = lane == 0 ? carry : up;
                    carry = cbc_wave_last(cb);                 /* (a short round is the last: not read again) */
                    uint4 p;
                    if constexpr (ALT)
                        p = xor4(blk_encrypt<NR, true>(lds, lanebase, rk, cb), prev);
                    else
                        p = xor4(cbc_aes_decrypt<NR>(lds, lanebase, rk, cb), prev);
                    if (live) gstore16(pdst + 16 * (size_t) i, p);
                }
                /* lane 0 reads what the wave's other lanes stored (file head) */
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                off += 16;                                                         /* :1572-1573 */
                if (lane == 0) {
                    len = cbc_check_padding(pdst, clen, pdst[clen - 1], ML, etm, correct);
                    if (etm) status = correct ? 0 : TLSREC_E_INVALID_MAC;
                }
            }
            status = __builtin_amdgcn_readfirstlane(status);   /* lane 0's: the wave leaves the loop together */
        }
        if (lane == 0 && !status && cidl) status = cbc_inner_plaintext(pdst, len, type);
    }
    if (lane == 0) {                                           /* the status is formed once */
        tlsrec_batch_res r;
        r.status = status;
        r.data_offset = off;
        r.data_len = len;
        r.type = (uint8_t) type;
        r.cid_len = 0;
        r.reserved[0] = r.reserved[1] = 0;
        a.res[rec] = r;
    }
}

} /* namespace tlsrec */

#endif /* TLSREC_CBC_WAVE_H */
