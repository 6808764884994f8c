/*
 * tlsrec_sha.h -- the word-wise SHA-2 compression the one-lane-per-connection
 * kernels share (tlsrec_kdf.h and its units: the TLS 1.2 / 1.3 ladders, the
 * exporters and the cookies;
 * transcript.hip: the running handshake hashes): round constants, the
 * per-hash traits S256 / S512 with their initial values, one round, one block.
 *
 * Device code only.  The constants are `__constant__ const` at namespace
 * scope (internal linkage), so every unit that includes this holds its own
 * copy and nothing is shared through the linker.
 */
#ifndef TLSREC_SHA_H
#define TLSREC_SHA_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tlsks {

/* ---------------- SHA-2 round constants (FIPS 180-4 4.2.2, 4.2.3) ------- */
__constant__ const uint32_t kK256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2 };

__constant__ const uint64_t kK512[80] = {
    0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL,
    0x3956c25bf348b538ULL, 0x59f111f1b605d019ULL, 0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL,
    0xd807aa98a3030242ULL, 0x12835b0145706fbeULL, 0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL,
    0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL, 0xc19bf174cf692694ULL,
    0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL, 0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL,
    0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL,
    0x983e5152ee66dfabULL, 0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL,
    0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL, 0x06ca6351e003826fULL, 0x142929670a0e6e70ULL,
    0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL, 0x53380d139d95b3dfULL,
    0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL,
    0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL, 0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL,
    0xd192e819d6ef5218ULL, 0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL,
    0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL, 0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL,
    0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL, 0x5b9cca4f7763e373ULL, 0x682e6ff3d6b2b8a3ULL,
    0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
    0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL,
    0xca273eceea26619cULL, 0xd186b8c721c0c207ULL, 0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL,
    0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL, 0x113f9804bef90daeULL, 0x1b710b35131c471bULL,
    0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL, 0x431d67c49c100d4cULL,
    0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL, 0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL };

__device__ __forceinline__ uint32_t ror32(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
__device__ __forceinline__ uint64_t ror64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

/* The per-hash traits of the word-wise kernels: the word type, the round
 * count, the constants, the four sigma functions and the initial value
 * (FIPS 180-4 5.3.3 for SHA-256; 5.3.4, SHA-384, for the SHA-512 compression --
 * the only SHA-512 family member TLS uses). */
struct S256 {
    typedef uint32_t W;
    enum { ROUNDS = 64 };
    static __device__ __forceinline__ W k(int i) { return kK256[i]; }
    static __device__ __forceinline__ W S0(W x) { return ror32(x, 2) ^ ror32(x, 13) ^ ror32(x, 22); }
    static __device__ __forceinline__ W S1(W x) { return ror32(x, 6) ^ ror32(x, 11) ^ ror32(x, 25); }
    static __device__ __forceinline__ W s0(W x) { return ror32(x, 7) ^ ror32(x, 18) ^ (x >> 3); }
    static __device__ __forceinline__ W s1(W x) { return ror32(x, 17) ^ ror32(x, 19) ^ (x >> 10); }
    static __device__ __forceinline__ W iv(int j)
    {
        const W t[8] = { 0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                         0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u };
        return t[j];
    }
};
struct S512 {
    typedef uint64_t W;
    enum { ROUNDS = 80 };
    static __device__ __forceinline__ W k(int i) { return kK512[i]; }
    static __device__ __forceinline__ W S0(W x) { return ror64(x, 28) ^ ror64(x, 34) ^ ror64(x, 39); }
    static __device__ __forceinline__ W S1(W x) { return ror64(x, 14) ^ ror64(x, 18) ^ ror64(x, 41); }
    static __device__ __forceinline__ W s0(W x) { return ror64(x, 1) ^ ror64(x, 8) ^ (x >> 7); }
    static __device__ __forceinline__ W s1(W x) { return ror64(x, 19) ^ ror64(x, 61) ^ (x >> 6); }
    static __device__ __forceinline__ W iv(int j)
    {
        const W t[8] = { 0xcbbb9d5dc1059ed8ULL, 0x629a292a367cd507ULL, 0x9159015a3070dd17ULL,
                         0x152fecd8f70e5939ULL, 0x67332667ffc00b31ULL, 0x8eb44a8768581511ULL,
                         0xdb0c2e0d64f98fa7ULL, 0x47b5481dbefa4fa4ULL };
        return t[j];
    }
};

/* One round with the working variables rotated by the (compile-time) round
 * index instead of moved: v[(0 - i) & 7] is a, ..., v[(7 - i) & 7] is h. */
template <class T> __device__ __forceinline__ void sha_round(typename T::W (&v)[8], int i, typename T::W kw)
{
    typedef typename T::W W;
    const W a = v[(0 - i) & 7], b = v[(1 - i) & 7], c = v[(2 - i) & 7];
    const W e = v[(4 - i) & 7], f = v[(5 - i) & 7], g = v[(6 - i) & 7];
    const W t1 = v[(7 - i) & 7] + T::S1(e) + (g ^ (e & (f ^ g))) + kw;
    const W t2 = T::S0(a) + ((a & b) | (c & (a | b)));
    v[(3 - i) & 7] += t1;
    v[(7 - i) & 7] = t1 + t2;
}

/* FIPS 180-4 6.2.2 / 6.4.2 on one block: 16 rounds unrolled per trip so that
 * every index into w[] and v[] is a constant (registers, no scratch), the
 * trips themselves rolled to keep the code of one call site to 16 rounds.
 * w[] is consumed (it becomes the last 16 schedule words). */
template <class T> __device__ __forceinline__ void sha_compress(typename T::W (&st)[8], typename T::W (&w)[16])
{
    typename T::W v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = st[i];
#pragma unroll
    for (int i = 0; i < 16; i++) sha_round<T>(v, i, T::k(i) + w[i]);
#pragma unroll 1
    for (int r = 16; r < T::ROUNDS; r += 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            w[i] += T::s0(w[(i + 1) & 15]) + w[(i + 9) & 15] + T::s1(w[(i + 14) & 15]);
            sha_round<T>(v, i, T::k(r + i) + w[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] += v[i];
}

}  // namespace tlsks

#endif /* TLSREC_SHA_H */
