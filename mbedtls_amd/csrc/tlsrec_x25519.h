/*
 * tlsrec_x25519.h -- X25519 (RFC 7748 section 5) as straight-line integer code
 * shared by the HIP kernels of x25519.hip and the host.
 *
 *   reference                                                    here
 *   psa_generate_key + psa_export_public_key
 *                          ssl_tls13_generic.c:1566-1582         x25519(out, k, 9)
 *   psa_raw_key_agreement  ssl_tls13_keys.c:1457,
 *                          ssl_tls12_server.c:3028               x25519(out, k, u)
 *
 * Field elements of GF(2^255 - 19) are ten signed limbs of alternately 26 and
 * 25 bits (radix 2^25.5): limb i has weight 2^ceil(25.5 i).  A product is 100
 * 32 x 32 -> 64 multiply-adds into ten 64-bit accumulators, the wrap past
 * 2^255 folded in as a factor 19 on one operand, then one carry pass; sums and
 * differences need no carry at all, because a limb has 6 spare bits.  Bounds, as
 * in the well-known analysis of this representation: fe_mul / fe_sq / fe_mul121666
 * take limbs up to 1.65 * 2^26 (even) and 1.65 * 2^25 (odd) in magnitude and give
 * limbs up to 1.01 * 2^25 and 1.01 * 2^24, so one fe_add or fe_sub of such
 * outputs may feed the next product, which is all the ladder asks.
 *
 * Constant time: the ladder's conditional swap is a mask; the
 * scalar is shifted through its top bit, so no index, address, branch or loop
 * bound depends on a scalar bit or a field value; the inversion is the fixed
 * chain for p - 2; fe_tobytes and the zero check are branch-free.
 *
 * Signed limbs are never shifted left (multiplied by a power of two instead),
 * and right shifts of negative values are arithmetic on every compiler this
 * builds with.
 */
#ifndef TLSREC_X25519_H
#define TLSREC_X25519_H

#include <stdint.h>

/* In the kernel everything is one body: a field element handed to a real call would have to
 * live in scratch memory.  The host pass has no such need and compiles faster without it. */
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define TLSREC_X_HD __host__ __device__ static inline __attribute__((always_inline))
#elif defined(__HIPCC__) || defined(__HIP__)
#define TLSREC_X_HD __host__ __device__ static inline
#else
#define TLSREC_X_HD static inline
#endif

namespace tlsrec {

typedef int32_t x25519_fe[10];

/* bit position of limb i, and its width */
TLSREC_X_HD constexpr int x25519_pos(int i) { return (51 * i + 1) / 2; }
TLSREC_X_HD constexpr int x25519_bits(int i) { return (i & 1) ? 25 : 26; }

TLSREC_X_HD void x25519_fe_set(x25519_fe h, int32_t v)
{
    h[0] = v;
#pragma unroll
    for (int i = 1; i < 10; i++) h[i] = 0;
}
TLSREC_X_HD void x25519_fe_copy(x25519_fe h, const x25519_fe f)
{
#pragma unroll
    for (int i = 0; i < 10; i++) h[i] = f[i];
}
TLSREC_X_HD void x25519_fe_add(x25519_fe h, const x25519_fe f, const x25519_fe g)
{
#pragma unroll
    for (int i = 0; i < 10; i++) h[i] = f[i] + g[i];
}
TLSREC_X_HD void x25519_fe_sub(x25519_fe h, const x25519_fe f, const x25519_fe g)
{
#pragma unroll
    for (int i = 0; i < 10; i++) h[i] = f[i] - g[i];
}
/* swap f and g where b == 1, leave them where b == 0 */
TLSREC_X_HD void x25519_fe_cswap(x25519_fe f, x25519_fe g, uint32_t b)
{
    const int32_t m = -(int32_t) b;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const int32_t x = (f[i] ^ g[i]) & m;
        f[i] ^= x;
        g[i] ^= x;
    }
}

/* one carry from limb i (B bits) into limb i + 1, rounding to nearest */
#define TLSREC_X_CARRY(i, B)                                                \
    do {                                                                    \
        const int64_t c = (h[i] + ((int64_t) 1 << ((B) - 1))) >> (B);       \
        h[(i) + 1] += c;                                                    \
        h[i] -= c * ((int64_t) 1 << (B));                                   \
    } while (0)

/* the carry pass after a product: ten 64-bit accumulators to ten limbs */
TLSREC_X_HD void x25519_fe_carry(x25519_fe out, int64_t (&h)[10])
{
    TLSREC_X_CARRY(0, 26);
    TLSREC_X_CARRY(4, 26);
    TLSREC_X_CARRY(1, 25);
    TLSREC_X_CARRY(5, 25);
    TLSREC_X_CARRY(2, 26);
    TLSREC_X_CARRY(6, 26);
    TLSREC_X_CARRY(3, 25);
    TLSREC_X_CARRY(7, 25);
    TLSREC_X_CARRY(4, 26);
    TLSREC_X_CARRY(8, 26);
    {
        /* limb 9 wraps to limb 0 with weight 2^255 = 19 */
        const int64_t c = (h[9] + ((int64_t) 1 << 24)) >> 25;
        h[0] += c * 19;
        h[9] -= c * ((int64_t) 1 << 25);
    }
    TLSREC_X_CARRY(0, 26);
#pragma unroll
    for (int i = 0; i < 10; i++) out[i] = (int32_t) h[i];
}

/* h = f g.  Term f_i g_j lands in limb (i + j) mod 10: doubled when i and j are both odd
 * (2^ceil(25.5 i) 2^ceil(25.5 j) is then twice the weight of limb i + j), times 19 when it
 * wraps.  The loops unroll; 2 f_i and 19 g_j are formed once each. */
TLSREC_X_HD void x25519_fe_mul(x25519_fe out, const x25519_fe f, const x25519_fe g)
{
    int32_t f2[10], g19[10];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        f2[i] = 2 * f[i];
        g19[i] = 19 * g[i];
    }
    int64_t h[10];
#pragma unroll
    for (int k = 0; k < 10; k++) {
        int64_t s = 0;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            const int j = (k - i + 10) % 10;
            const int32_t a = ((i & 1) && (j & 1)) ? f2[i] : f[i];
            const int32_t b = (i + j >= 10) ? g19[j] : g[j];
            s += (int64_t) a * b;
        }
        h[k] = s;
    }
    x25519_fe_carry(out, h);
}

/* h = f^2: the 55 terms i <= j, the off-diagonal ones doubled */
TLSREC_X_HD void x25519_fe_sq(x25519_fe out, const x25519_fe f)
{
    int32_t f2[10], f19[10], f38[10];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        f2[i] = 2 * f[i];
        f19[i] = 19 * f[i];
        f38[i] = (i & 1) ? 38 * f[i] : 0;       /* 38 f_i fits 32 bits for the odd (25-bit) limbs only */
    }
    int64_t h[10];
#pragma unroll
    for (int k = 0; k < 10; k++) {
        int64_t s = 0;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            const int j = (k - i + 10) % 10;
            if (i > j) continue;
            const bool odd = (i & 1) && (j & 1), wrap = i + j >= 10;
            const int32_t a = i != j ? f2[i] : f[i];
            const int32_t b = wrap ? (odd ? f38[j] : f19[j]) : (odd ? f2[j] : f[j]);
            s += (int64_t) a * b;
        }
        h[k] = s;
    }
    x25519_fe_carry(out, h);
}

/* h = f^(2^n), n >= 1 and a constant of the caller */
TLSREC_X_HD void x25519_fe_sqn(x25519_fe h, const x25519_fe f, int n)
{
    x25519_fe_sq(h, f);
#pragma unroll 1
    for (int i = 1; i < n; i++) x25519_fe_sq(h, h);
}

/* h = 121666 f, (A + 2) / 4 of the curve */
TLSREC_X_HD void x25519_fe_mul121666(x25519_fe out, const x25519_fe f)
{
    int64_t h[10];
#pragma unroll
    for (int i = 0; i < 10; i++) h[i] = (int64_t) f[i] * 121666;
    x25519_fe_carry(out, h);
}

/* out = z^(p - 2) = z^(2^255 - 21), the fixed addition chain: 254 squarings, 11 products */
TLSREC_X_HD void x25519_fe_invert(x25519_fe out, const x25519_fe z)
{
    x25519_fe t0, t1, t2, t3;
    x25519_fe_sq(t0, z);             /* 2 */
    x25519_fe_sqn(t1, t0, 2);        /* 8 */
    x25519_fe_mul(t1, z, t1);        /* 9 */
    x25519_fe_mul(t0, t0, t1);       /* 11 */
    x25519_fe_sq(t2, t0);            /* 22 */
    x25519_fe_mul(t1, t1, t2);       /* 2^5 - 1 */
    x25519_fe_sqn(t2, t1, 5);
    x25519_fe_mul(t1, t2, t1);       /* 2^10 - 1 */
    x25519_fe_sqn(t2, t1, 10);
    x25519_fe_mul(t2, t2, t1);       /* 2^20 - 1 */
    x25519_fe_sqn(t3, t2, 20);
    x25519_fe_mul(t2, t3, t2);       /* 2^40 - 1 */
    x25519_fe_sqn(t2, t2, 10);
    x25519_fe_mul(t1, t2, t1);       /* 2^50 - 1 */
    x25519_fe_sqn(t2, t1, 50);
    x25519_fe_mul(t2, t2, t1);       /* 2^100 - 1 */
    x25519_fe_sqn(t3, t2, 100);
    x25519_fe_mul(t2, t3, t2);       /* 2^200 - 1 */
    x25519_fe_sqn(t2, t2, 50);
    x25519_fe_mul(t1, t2, t1);       /* 2^250 - 1 */
    x25519_fe_sqn(t1, t1, 5);        /* 2^255 - 2^5 */
    x25519_fe_mul(out, t1, t0);      /* 2^255 - 21 */
    x25519_fe_set(t0, 0);
    x25519_fe_set(t1, 0);
    x25519_fe_set(t2, 0);
    x25519_fe_set(t3, 0);
}

/* decodeUCoordinate: eight little-endian words to limbs, bit 255 dropped; a value in
 * 2^255 - 19 .. 2^255 - 1 is taken as it is and reduced by the arithmetic */
TLSREC_X_HD void x25519_fe_frombytes(x25519_fe h, const uint32_t (&w)[8])
{
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const int p = x25519_pos(i), q = p >> 5, s = p & 31;
        uint64_t v = w[q];
        if (q + 1 < 8) v |= (uint64_t) w[q + 1] << 32;
        h[i] = (int32_t) ((uint32_t) (v >> s) & ((1u << x25519_bits(i)) - 1));
    }
}

/* the canonical encoding: the value reduced to 0 .. p - 1, without a branch on it */
TLSREC_X_HD void x25519_fe_tobytes(uint32_t (&w)[8], const x25519_fe f)
{
    int32_t h[10];
#pragma unroll
    for (int i = 0; i < 10; i++) h[i] = f[i];
    /* q = 1 where the value is at least p: the carry out of value + 19 */
    int32_t q = (19 * h[9] + ((int32_t) 1 << 24)) >> 25;
#pragma unroll
    for (int i = 0; i < 10; i++) q = (h[i] + q) >> x25519_bits(i);
    h[0] += 19 * q;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const int32_t c = h[i] >> x25519_bits(i);
        if (i < 9) h[i + 1] += c;            /* the carry out of limb 9 is the 2^255 q that goes */
        h[i] -= c * ((int32_t) 1 << x25519_bits(i));
    }
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const int p = x25519_pos(i), k = p >> 5, s = p & 31;
        const uint64_t v = (uint64_t) (uint32_t) h[i] << s;
        w[k] |= (uint32_t) v;
        if (k + 1 < 8) w[k + 1] |= (uint32_t) (v >> 32);
    }
#pragma unroll
    for (int i = 0; i < 10; i++) h[i] = 0;
}

/* out = X25519(k, u), all three as eight little-endian 32-bit words; k is clamped here
 * (decodeScalar25519).  BASE: u is the base point 9 and `u` is not looked at.  Returns 1,
 * or 0 where out is all zero (RFC 7748 section 6.1, RFC 8446 section 7.4.2): the OR of the
 * eight output words, without a branch.  Every secret the function held is set to zero. */
template <bool BASE> TLSREC_X_HD uint32_t x25519(uint32_t (&out)[8], const uint32_t (&k)[8], const uint32_t (&u)[8])
{
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = k[i];
    e[0] &= 0xfffffff8u;
    e[7] = (e[7] & 0x7fffffffu) | 0x40000000u;
    /* bit 254 to the top: each step takes the top bit and shifts the scalar up by one */
#pragma unroll
    for (int i = 7; i > 0; i--) e[i] = (e[i] << 1) | (e[i - 1] >> 31);
    e[0] <<= 1;

    x25519_fe x1, x2, z2, x3, z3, t0, t1;
    if (BASE) x25519_fe_set(x1, 9);
    else x25519_fe_frombytes(x1, u);
    x25519_fe_set(x2, 1);
    x25519_fe_set(z2, 0);
    x25519_fe_copy(x3, x1);
    x25519_fe_set(z3, 1);

    uint32_t swap = 0;
#pragma unroll 1
    for (int t = 254; t >= 0; t--) {
        const uint32_t b = e[7] >> 31;
#pragma unroll
        for (int i = 7; i > 0; i--) e[i] = (e[i] << 1) | (e[i - 1] >> 31);
        e[0] <<= 1;
        swap ^= b;
        x25519_fe_cswap(x2, x3, swap);
        x25519_fe_cswap(z2, z3, swap);
        swap = b;

        x25519_fe_sub(t0, x3, z3);
        x25519_fe_sub(t1, x2, z2);
        x25519_fe_add(x2, x2, z2);
        x25519_fe_add(z2, x3, z3);
        x25519_fe_mul(z3, t0, x2);
        x25519_fe_mul(z2, z2, t1);
        x25519_fe_sq(t0, t1);
        x25519_fe_sq(t1, x2);
        x25519_fe_add(x3, z3, z2);
        x25519_fe_sub(z2, z3, z2);
        x25519_fe_mul(x2, t1, t0);
        x25519_fe_sub(t1, t1, t0);
        x25519_fe_sq(z2, z2);
        x25519_fe_mul121666(z3, t1);
        x25519_fe_sq(x3, x3);
        x25519_fe_add(t0, t0, z3);
        x25519_fe_mul(z3, x1, z2);
        x25519_fe_mul(z2, t1, t0);
    }
    x25519_fe_cswap(x2, x3, swap);
    x25519_fe_cswap(z2, z3, swap);

    x25519_fe_invert(z2, z2);
    x25519_fe_mul(x2, x2, z2);
    x25519_fe_tobytes(out, x2);

    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) any |= out[i];
    const uint32_t ok = (any | (0u - any)) >> 31;

#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = 0;
    swap = 0;
    x25519_fe_set(x1, 0);
    x25519_fe_set(x2, 0);
    x25519_fe_set(z2, 0);
    x25519_fe_set(x3, 0);
    x25519_fe_set(z3, 0);
    x25519_fe_set(t0, 0);
    x25519_fe_set(t1, 0);
    return ok;
}

}  // namespace tlsrec

#undef TLSREC_X_CARRY
#endif /* TLSREC_X25519_H */
