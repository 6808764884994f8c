/*
 * aes_ghash_n.h -- the NB-blocks-per-lane AES-CTR + GHASH step of the ILP and
 * hybrid probes (ilp_probe.hip, hybrid_probe.hip).  The library runs one block
 * per lane and step (aes_ghash, tlsrec_device.h); this form, and the pointer-
 * relative table read it uses, live with the probes that measure it.
 */
#ifndef TLSREC_PROBE_AES_GHASH_N_H
#define TLSREC_PROBE_AES_GHASH_N_H

#include "tlsrec_device.h"

namespace tlsrec {

/* Part of gmul: the table reads of bytes e0 .. e0+NE-1 of 32-bit word d of y. */
template <int PI, int NE = 4>
__device__ __forceinline__ void gmul_word(const uint8_t *lds, uint32_t wd, int d, uint4 &acc, int e0 = 0)
{
#pragma unroll
    for (int i = 0; i < NE; i++) {
        const int e = e0 + i;
        const int b = 4 * d + e;
        uint32_t ahi = (e == 0) ? (wd & 0xf0u) : ((wd >> (8 * e)) & 0xf0u);
        uint32_t alo = (e == 0) ? ((wd << 4) & 0xf0u) : ((wd >> (8 * e - 4)) & 0xf0u);
        uint4 th = *reinterpret_cast<const uint4 *>(lds + ahi + PI * 8192 + (2 * b) * 256);
        uint4 tl = *reinterpret_cast<const uint4 *>(lds + alo + PI * 8192 + (2 * b + 1) * 256);
        acc.x = xor3(acc.x, th.x, tl.x);
        acc.y = xor3(acc.y, th.y, tl.y);
        acc.z = xor3(acc.z, th.z, tl.z);
        acc.w = xor3(acc.w, th.w, tl.w);
    }
}

/* NB independent counter blocks of one record and NB independent GHASH
 * multiplies per call (NB Horner chains per lane), phase-interleaved as in
 * aes_ghash: chain b's group g of 4 table reads follows AES round 2 + g. */
template <int NR, int AES_OFF, int PI, int NB, typename RK>
__device__ __forceinline__ void aes_ghash_n(const uint8_t *lds, uint32_t lb, RK rk, const CtrCache &cc,
                                            const uint32_t (&ctrw)[NB], const uint4 (&y)[NB], uint4 (&ks)[NB],
                                            uint4 (&prod)[NB])
{
    static_assert(NR >= 10, "rounds 2..9 carry the GHASH groups");
#define TA(x, k) tlook<AES_OFF>(lds, (x), lb, (k), 0)
#define TB(x, k) tlook<AES_OFF>(lds, (x), lb, (k), 1)
    uint32_t s[NB][4];
    uint32_t w[NB][4];
    uint4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const uint32_t w3 = ctrw[b] ^ rk[3];
        const uint32_t t0 = rotl16(cc.k0r ^ TB(w3, 3));
        const uint32_t t1 = rotl16(cc.k1r ^ TA(w3, 2));
        s[b][0] = xor3(TA(t0, 0), TB(t1, 1), cc.d0);
        s[b][1] = xor3(TA(t1, 0), cc.d1, rotl16(TB(t0, 3)));
        s[b][2] = rotl16(xor3(TA(t0, 2), TB(t1, 3), cc.d2r));
        s[b][3] = xor3(TB(t0, 1), cc.d3, rotl16(TA(t1, 2)));
        w[b][0] = y[b].x; w[b][1] = y[b].y; w[b][2] = y[b].z; w[b][3] = y[b].w;
        acc[b] = make_uint4(0, 0, 0, 0);
    }
#undef TA
#undef TB
#pragma unroll
    for (int r = 2; r < NR; r++) {
        if (r > 2) {
#pragma unroll
            for (int b = 0; b < NB; b++) aes_round<AES_OFF>(lds, lb, rk, r, s[b][0], s[b][1], s[b][2], s[b][3]);
        }
        const int g = r - 2;
        if (g < 8) {
#pragma unroll
            for (int b = 0; b < NB; b++) gmul_word<PI, 2>(lds, w[b][g >> 1], g >> 1, acc[b], 2 * (g & 1));
#pragma unroll
            for (int b = 0; b < NB; b++) {
                asm volatile("" : "+v"(s[b][0]), "+v"(s[b][1]), "+v"(s[b][2]), "+v"(s[b][3]), "+v"(acc[b].x),
                             "+v"(acc[b].y), "+v"(acc[b].z), "+v"(acc[b].w));
                if (g < 2) asm volatile("" : "+v"(w[b][1]), "+v"(w[b][2]), "+v"(w[b][3]));
                else if (g < 4) asm volatile("" : "+v"(w[b][2]), "+v"(w[b][3]));
                else if (g < 6) asm volatile("" : "+v"(w[b][3]));
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
        uint32_t o[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint32_t a = tlook<AES_OFF>(lds, s[b][c], lb, 0, 0);
            uint32_t bb = tlook<AES_OFF>(lds, s[b][(c + 1) & 3], lb, 1, 0);
            uint32_t d2 = tlook<AES_OFF>(lds, s[b][(c + 2) & 3], lb, 2, 0);
            uint32_t d3 = tlook<AES_OFF>(lds, s[b][(c + 3) & 3], lb, 3, 0);
            uint32_t lo = __builtin_amdgcn_perm(bb, a, 0x0C0C0501u);
            uint32_t hi = __builtin_amdgcn_perm(d3, d2, 0x06020C0Cu);
            o[c] = __builtin_amdgcn_bitop3_b32(lo, hi, rk[4 * NR + c], 0x56);
        }
        ks[b] = make_uint4(o[0], o[1], o[2], o[3]);
        prod[b] = acc[b];
    }
}

} /* namespace tlsrec */

#endif /* TLSREC_PROBE_AES_GHASH_N_H */
