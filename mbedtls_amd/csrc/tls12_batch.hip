/*
 * tls12_batch.hip -- the TLS 1.2 / DTLS 1.2 handshake of library/ssl_tls.c in
 * batches, one connection per lane, on the word-wise blocks of tlsrec_kdf.h:
 *
 *   reference                                        here
 *   ssl_compute_master                :6251-6452     tlsrec_tls12_batch_compute_master
 *   ssl_calc_finished_tls_generic     :7209-7261,
 *   mbedtls_ssl_parse_finished        :7530          tlsrec_tls12_batch_verify_data
 *   tls_prf(.., "key expansion", ..)  :7750          tlsrec_tls12_keytab_derive, _derive_cbc
 *   key-block split                   :7858-7892     in the kernels; tlsrec_tls12_split_key_block,
 *                                                    _split_key_block_cbc (host only)
 *
 * The single-shot forms (tlsrec_tls_prf, tlsrec_tls12_make_keys, ...) are in
 * keysched.hip, the keying-material exporter in exporter.hip.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_frame.h"     /* tlsrec_cipher_keylen, tlsrec_cipher_taglen */
#include "tlsrec_internal.h"
#include "tlsrec_kdf.h"

namespace tlsks {

/* ---- the PRF of RFC 5246 section 5 for fixed shapes ----------------------
 * The master secret (ssl_compute_master, ssl_tls.c:6251-6452), the Finished
 * verify_data (ssl_calc_finished_tls_generic, :7209-7261, with the
 * constant-time check of mbedtls_ssl_parse_finished, :7530) and the key block
 * (:7750) are all PRF(secret, label, seed) = P_hash(secret, label || seed) cut
 * to 48, 12 or the key block's bytes: two midstates of the secret, then per
 * iteration A(i) = HMAC(A(i-1)) and HMAC(A(i) || label || seed).
 *
 * label || seed, N bytes in the cells S[]:
 *   "master secret" | "key expansion" || randbytes  13 + 64 = 77
 *   "extended master secret" || session_hash  22 + 32 = 54, 22 + 48 = 70
 *   "client finished" | "server finished" || transcript hash  15 + 32 = 47, 15 + 48 = 63
 * N is a constant of the instantiation, so the padding and the length word of
 * every block are constants.  Compressions per connection:
 *   A(1): 1, or 2 where N + 9 > 64 (SHA-256, 77);  A(i > 1): 1;  each outer hash: 1
 *   HMAC(A || S): Hash.length + N bytes, 2 inner blocks, or 1 where it pads
 *   into one (SHA-384, 48 + 63 + 17 = 128)
 *   master, SHA-256: 2 + (3 | 2) + 3 + 2 + 3 = 13 | 12, and 2 | 3 more where the
 *   premaster is longer than the block and is hashed first;  SHA-384: 2 + 2 + 3 = 7
 *   verify_data: SHA-256 2 + 2 + 3 = 7;  SHA-384 2 + 2 + 2 = 6
 *   key block, n = ceil(out_len / H): SHA-256 5n + 3, SHA-384 5n + 2 */

/* The first OUTC cells of P_hash over the N bytes of S under the midstates ip / op. */
template <class T, int N, int OUTC>
__device__ __forceinline__ void tls12_p_hash(const typename T::W (&ip)[8], const typename T::W (&op)[8],
                                             const uint32_t (&S)[20], uint32_t (&out)[OUTC])
{
    typedef typename T::W W;
    constexpr int ITERS = (4 * OUTC + T::HB - 1) / T::HB;
    constexpr int NC = T::HC + 20, L = T::HB + N;      /* A || S */
    static_assert(N <= 80 && N + 1 + T::LENB <= 2 * T::BB && L + 1 + T::LENB <= 2 * T::BB, "one or two inner blocks");
    W w[16], st[8], A[T::HW];
    uint32_t C[NC];
#pragma unroll
    for (int j = 0; j < T::HC; j++) C[j] = 0;
#pragma unroll
    for (int j = 0; j < 20; j++) C[T::HC + j] = S[j];
#pragma unroll
    for (int j = 0; j < T::HW; j++) A[j] = 0;
#pragma unroll 1
    for (int it = 0; it < ITERS; it++) {
        /* A(it + 1) = HMAC(A(it)); A(0) is S */
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        if (it == 0) {
            msg_block<T, 20>(w, S, N, 0);
            sha_compress<typename T::S>(st, w);
            if constexpr (N + 1 + T::LENB > T::BB) {
                msg_block<T, 20>(w, S, N, 1);
                sha_compress<typename T::S>(st, w);
            }
        } else {
            digest_block<T>(w, A);
            sha_compress<typename T::S>(st, w);
        }
        hmac_outer<T>(op, st, A);
        /* output block = HMAC(A || S) */
#pragma unroll
        for (int c = 0; c < T::HC; c++) C[c] = cell<T, T::HW>(A, c);
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        msg_block<T, NC>(w, C, L, 0);
        sha_compress<typename T::S>(st, w);
        if constexpr (L + 1 + T::LENB > T::BB) {
            msg_block<T, NC>(w, C, L, 1);
            sha_compress<typename T::S>(st, w);
        }
        W D[T::HW];
        hmac_outer<T>(op, st, D);
#pragma unroll
        for (int q = 0; q < ITERS; q++) {
            if (it == q) {
#pragma unroll
                for (int c = 0; c < T::HC; c++)
                    if (q * T::HC + c < OUTC) out[q * T::HC + c] = cell<T, T::HW>(D, c);
            }
        }
#pragma unroll
        for (int j = 0; j < T::HW; j++) D[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = 0;
#pragma unroll
    for (int j = 0; j < T::HW; j++) A[j] = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int j = 0; j < NC; j++) C[j] = 0;
}

/* The key block under SHA-256, P_SHA256(master, "key expansion" || randbytes),
 * written out by hand: the same computation as tls12_p_hash<L256, 77, .>, kept
 * because its one loop body, which blends the first and the later A(i) blocks
 * with selects, takes fewer registers than the generic loop's two code paths
 * (DESIGN.md 3.19).  KB receives 8 words per iteration, ITERS = ceil(out_len / 32).
 * The blocks carry their padding as constants, so S[19] holds the seed's last
 * byte and the 0x80 that follows it wherever the seed ends a message. */
template <int ITERS, int KBW>
__device__ __forceinline__ void tls12_expand_sha256(const uint32_t (&M)[12], const uint32_t (&R)[16],
                                                    uint32_t (&KB)[KBW])
{
    static_assert(ITERS * 8 <= KBW, "key block holds every iteration's digest");
    const uint32_t HMAC_LEN = (64 + 32) * 8;     /* bits of key block || 32-byte digest */
    uint32_t S[20], w[16], ip[8], op[8], st[8], A[8];
    tls12_seed77(S, 0x6b657920u, 0x65787061u, 0x6e73696fu, 0x6e000000u, R);     /* "key expansion" */
    S[19] |= 0x00800000u;
    /* midstates: one block of master ^ pad, master zero-padded to 64 bytes (RFC 2104) */
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = (j < 12 ? M[j] : 0u) ^ 0x36363636u;
#pragma unroll
    for (int j = 0; j < 8; j++) ip[j] = S256::iv(j);
    sha_compress<S256>(ip, w);
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = (j < 12 ? M[j] : 0u) ^ 0x5c5c5c5cu;
#pragma unroll
    for (int j = 0; j < 8; j++) op[j] = S256::iv(j);
    sha_compress<S256>(op, w);
    /* outer hash of an HMAC: opad midstate over the 32-byte inner digest in st */
    auto outer = [&](uint32_t (&dst)[8]) {
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = st[j];
        w[8] = 0x80000000u;
#pragma unroll
        for (int j = 9; j < 15; j++) w[j] = 0;
        w[15] = HMAC_LEN;
#pragma unroll
        for (int j = 0; j < 8; j++) dst[j] = op[j];
        sha_compress<S256>(dst, w);
    };
#pragma unroll
    for (int j = 0; j < 8; j++) A[j] = 0;
#pragma unroll 1
    for (int it = 0; it < ITERS; it++) {
        /* A(it + 1) = HMAC(A(it)); A(0) is the seed, whose 77 bytes take a second block */
        const bool first = it == 0;
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = first ? S[j] : A[j];
        w[8] = first ? S[8] : 0x80000000u;
#pragma unroll
        for (int j = 9; j < 15; j++) w[j] = first ? S[j] : 0u;
        w[15] = first ? S[15] : HMAC_LEN;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        sha_compress<S256>(st, w);
        if (first) {
            w[0] = S[16]; w[1] = S[17]; w[2] = S[18]; w[3] = S[19];
#pragma unroll
            for (int j = 4; j < 15; j++) w[j] = 0;
            w[15] = (64 + 77) * 8;
            sha_compress<S256>(st, w);
        }
        outer(A);
        /* output block = HMAC(A || seed): 109 bytes, 64 + 45 */
#pragma unroll
        for (int j = 0; j < 8; j++) { w[j] = A[j]; w[8 + j] = S[j]; }
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        sha_compress<S256>(st, w);
#pragma unroll
        for (int j = 0; j < 12; j++) w[j] = S[8 + j];
        w[12] = 0; w[13] = 0; w[14] = 0;
        w[15] = (64 + 109) * 8;
        sha_compress<S256>(st, w);
        uint32_t D[8];
        outer(D);
#pragma unroll
        for (int q = 0; q < ITERS; q++) {
            if (it == q) {
#pragma unroll
                for (int j = 0; j < 8; j++) KB[8 * q + j] = D[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) D[j] = 0;
    }
    /* the reference zeroizes keyblk and the PSA operation; nothing of the chain stays behind */
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; st[j] = 0; A[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int j = 0; j < 20; j++) S[j] = 0;
}

/* ---- key expansion ---------------------------------------------------------
 * The first KBW cells of PRF(master, "key expansion", server_random ||
 * client_random) for the connection at conn (master[48] || randbytes[64]):
 * seven 16-byte loads, or bytes when the array is not 16-byte aligned.  Every
 * shape is fixed (48-byte key, 77-byte seed, at most 88 bytes out for an AEAD
 * suite and 160 for a CBC + HMAC one).  Under SHA-384 this is tls12_p_hash;
 * SHA-256 keeps its hand-written expander above.  The reference zeroizes keyblk
 * and the PSA operation; nothing of the chain stays behind here either. */
template <class T, int KBW>
__device__ __forceinline__ void tls12_key_block(const tlsrec_tls12_conn *conn, bool aligned, uint32_t (&KB)[KBW])
{
    static_assert(sizeof(tlsrec_tls12_conn) == 112 && offsetof(tlsrec_tls12_conn, randbytes) == 48,
                  "tlsrec_tls12_conn layout");
    typedef typename T::W W;
    const uint8_t *c = reinterpret_cast<const uint8_t *>(conn);
    uint32_t M[12], R[16];
    load_cells<12>(c, aligned, M);
    load_cells<16>(c + 48, aligned, R);
    if constexpr (sizeof(W) == 4) {
        tls12_expand_sha256<KBW / 8>(M, R, KB);
    } else {
        uint32_t S[20];
        W kb[16], ip[8], op[8];
        msg_block<T, 12, NO_PAD>(kb, M, 48, 0);
        hmac_mid_block<T>(kb, ip, op);
        tls12_seed77(S, 0x6b657920u, 0x65787061u, 0x6e73696fu, 0x6e000000u, R);     /* "key expansion" */
        tls12_p_hash<T, 77, KBW>(ip, op, S, KB);
#pragma unroll
        for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
        for (int j = 0; j < 20; j++) S[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 12; j++) M[j] = 0;
}

struct Tls12Args {
    const tlsrec_tls12_conn *conns;
    tlsrec_key_material *out;     /* staging area of slot `first`: 2 records per connection */
    uint32_t count, cipher, taglen, aligned;
};

/* One lane per connection; KL / IVL = the cipher's key length and TLS 1.2
 * fixed_ivlen, so the split of the key block (ssl_tls.c:7858-7892) indexes
 * registers with constants. */
template <class T, int KL, int IVL> __global__ void __launch_bounds__(64) tls12_derive_kernel(Tls12Args a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    constexpr int OUT = 2 * KL + 2 * IVL, KBW = (OUT + T::HB - 1) / T::HB * T::HC;
    static_assert(KL % 4 == 0 && IVL % 4 == 0, "key block shape");
    uint32_t KB[KBW];
    tls12_key_block<T>(a.conns + i, a.aligned != 0, KB);
    /* tlsrec_key_material: cipher, tls_minor 3, fixed_ivlen, taglen | granularity 0, reserved |
     * iv[16] | key[32]; client_write first, then server_write */
    const uint32_t head = a.cipher | (3u << 8) | ((uint32_t) IVL << 16) | (a.taglen << 24);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + 2 * (size_t) i);
#pragma unroll
    for (int side = 0; side < 2; side++) {
        uint32_t km[16];
        km[0] = head;
#pragma unroll
        for (int j = 1; j < 16; j++) km[j] = 0;
#pragma unroll
        for (int j = 0; j < IVL / 4; j++) km[4 + j] = __builtin_bswap32(KB[2 * KL / 4 + side * (IVL / 4) + j]);
#pragma unroll
        for (int j = 0; j < KL / 4; j++) km[8 + j] = __builtin_bswap32(KB[side * (KL / 4) + j]);
#pragma unroll
        for (int k = 0; k < 4; k++) dst[4 * side + k] = make_uint4(km[4 * k], km[4 * k + 1], km[4 * k + 2], km[4 * k + 3]);
#pragma unroll
        for (int j = 0; j < 16; j++) km[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < KBW; j++) KB[j] = 0;
}

struct Tls12CbcArgs {
    const tlsrec_tls12_conn *conns;
    tlsrec_cbc_key_material *out;     /* CBC staging area of slot `first`: 2 records per connection */
    uint32_t count, head, aligned;    /* head: cipher | tls_minor 3 | mac | etm, the first word of a record */
};

/* The CBC + HMAC suites: the key block is client_mac | server_mac | client_key
 * | server_key (ssl_tls.c:7858-7886, mac_key_len != 0; TLS 1.2 carries the CBC
 * IV in each record, so no IV is derived), 72 to 160 bytes = 3 to 5 P_SHA256 or
 * 2 to 4 P_SHA384 iterations.  One lane per connection as above; KL / ML = the
 * key and MAC key lengths, all multiples of 4 bytes, so the split indexes
 * registers with constants.  Each side is one tlsrec_cbc_key_material (128
 * bytes: head, 44 reserved bytes, key at byte 48, mac_key at byte 80). */
template <class T, int KL, int ML> __global__ void __launch_bounds__(64) tls12_derive_cbc_kernel(Tls12CbcArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    constexpr int OUT = 2 * ML + 2 * KL, KBW = (OUT + T::HB - 1) / T::HB * T::HC;
    static_assert(KL % 4 == 0 && KL <= 32 && ML % 4 == 0 && ML <= 48, "key block shape");
    static_assert(sizeof(tlsrec_cbc_key_material) == 128 && offsetof(tlsrec_cbc_key_material, key) == 48 &&
                  offsetof(tlsrec_cbc_key_material, mac_key) == 80, "tlsrec_cbc_key_material layout");
    uint32_t KB[KBW];
    tls12_key_block<T>(a.conns + i, a.aligned != 0, KB);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + 2 * (size_t) i);
#pragma unroll
    for (int side = 0; side < 2; side++) {
        uint32_t km[32];
        km[0] = a.head;
#pragma unroll
        for (int j = 1; j < 32; j++) km[j] = 0;
#pragma unroll
        for (int j = 0; j < KL / 4; j++) km[12 + j] = __builtin_bswap32(KB[2 * ML / 4 + side * (KL / 4) + j]);
#pragma unroll
        for (int j = 0; j < ML / 4; j++) km[20 + j] = __builtin_bswap32(KB[side * (ML / 4) + j]);
#pragma unroll
        for (int k = 0; k < 8; k++) dst[8 * side + k] = make_uint4(km[4 * k], km[4 * k + 1], km[4 * k + 2], km[4 * k + 3]);
#pragma unroll
        for (int j = 0; j < 32; j++) km[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < KBW; j++) KB[j] = 0;
}

/* ---- master secret, Finished verify_data ------------------------------------ */

struct Tls12MasterArgs {
    const tlsrec_tls12_pms_conn *conns;
    tlsrec_tls12_conn *out;
    uint32_t count, pms_len, aligned;     /* AL_CONNS conns, AL_AUX out */
};

/* EMS: "extended master secret" over the session hash (RFC 7627 section 4,
 * ssl_tls.c:6284-6305), else "master secret" over randbytes (:6269).  The
 * premaster is the HMAC key: zero-padded to the block, or under SHA-256 its
 * digest where it is longer than 64 bytes (RFC 2104; two inner blocks up to
 * 119 bytes, three from 120).  Only the 16-byte groups that hold premaster
 * bytes are loaded. */
template <class T, bool EMS> __global__ void __launch_bounds__(64) tls12_master_kernel(Tls12MasterArgs a)
{
    typedef typename T::W W;
    static_assert(sizeof(tlsrec_tls12_pms_conn) == 240 && offsetof(tlsrec_tls12_pms_conn, randbytes) == 128 &&
                  offsetof(tlsrec_tls12_pms_conn, session_hash) == 192 && sizeof(tlsrec_tls12_conn) == 112,
                  "tlsrec_tls12_pms_conn / tlsrec_tls12_conn layout");
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint8_t *conn = reinterpret_cast<const uint8_t *>(a.conns + i);
    const bool cal = (a.aligned & AL_CONNS) != 0;
    const uint32_t n = a.pms_len;
    W ip[8], op[8], w[16];
    /* every load of the connection is issued before the first compression: one wait on memory, not three */
    uint32_t R[16], S[20], X[12], Hs[EMS ? (int) T::HC : 1];
    load_cells<16>(conn + 128, cal, R);
    if constexpr (EMS) load_cells<T::HC>(conn + 192, cal, Hs);
    {
        uint32_t P[32];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uint32_t g[4] = { 0u, 0u, 0u, 0u };
            if ((uint32_t) (16 * k) < n) load_cells<4>(conn + 16 * k, cal, g);
#pragma unroll
            for (int j = 0; j < 4; j++) { P[4 * k + j] = g[j]; g[j] = 0; }
        }
        W kb[16];
        bool hashed = false;
        if constexpr (sizeof(W) == 4) hashed = n > T::BB;
        if (hashed) {
            W st[8];
#pragma unroll
            for (int j = 0; j < 8; j++) st[j] = T::iv(j);
            msg_block<T, 32, 0>(w, P, n, 0);
            sha_compress<typename T::S>(st, w);
            msg_block<T, 32, 0>(w, P, n, 1);
            sha_compress<typename T::S>(st, w);
            if (n + 1 + T::LENB > 2 * T::BB) {
                msg_block<T, 32, 0>(w, P, n, 2);
                sha_compress<typename T::S>(st, w);
            }
#pragma unroll
            for (int j = 0; j < 16; j++) kb[j] = j < T::HW ? st[j] : (W) 0;
#pragma unroll
            for (int j = 0; j < 8; j++) st[j] = 0;
        } else {
            msg_block<T, 32, NO_PAD>(kb, P, n, 0);
        }
#pragma unroll
        for (int j = 0; j < 32; j++) P[j] = 0;
        hmac_mid_block<T>(kb, ip, op);
    }
    constexpr int N = EMS ? 22 + (int) T::HB : 77;
    if constexpr (EMS) {
        S[0] = 0x65787465u;      /* "exte" */
        S[1] = 0x6e646564u;      /* "nded" */
        S[2] = 0x206d6173u;      /* " mas" */
        S[3] = 0x74657220u;      /* "ter " */
        S[4] = 0x73656372u;      /* "secr" */
        S[5] = 0x65740000u | (Hs[0] >> 16);     /* "et" */
#pragma unroll
        for (int k = 1; k < T::HC; k++) S[5 + k] = (Hs[k - 1] << 16) | (Hs[k] >> 16);
        S[5 + T::HC] = Hs[T::HC - 1] << 16;
#pragma unroll
        for (int k = 6 + T::HC; k < 20; k++) S[k] = 0;
    } else {
        tls12_seed77(S, 0x6d617374u, 0x65722073u, 0x65637265u, 0x74000000u, R);     /* "master secret" */
    }
    tls12_p_hash<T, N, 12>(ip, op, S, X);
    /* master || server_random || client_random: the swap of ssl_tls.c:6479-6488 */
    uint32_t o[28];
#pragma unroll
    for (int c = 0; c < 12; c++) o[c] = __builtin_bswap32(X[c]);
#pragma unroll
    for (int c = 0; c < 8; c++) { o[12 + c] = __builtin_bswap32(R[8 + c]); o[20 + c] = __builtin_bswap32(R[c]); }
    if (a.aligned & AL_AUX) {
        uint4 *q = reinterpret_cast<uint4 *>(a.out + i);
#pragma unroll
        for (int k = 0; k < 7; k++) q[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else {
        uint8_t *b = reinterpret_cast<uint8_t *>(a.out + i);
#pragma unroll
        for (int c = 0; c < 28; c++) {
            b[4 * c] = (uint8_t) o[c]; b[4 * c + 1] = (uint8_t) (o[c] >> 8);
            b[4 * c + 2] = (uint8_t) (o[c] >> 16); b[4 * c + 3] = (uint8_t) (o[c] >> 24);
        }
    }
#pragma unroll
    for (int j = 0; j < 12; j++) { X[j] = 0; o[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int j = 0; j < 20; j++) S[j] = 0;
}

enum { AL_VERIFY = AL_AUX, AL_OFFERED12 = AL_TRAFFIC };

struct Tls12FinishedArgs {
    const tlsrec_tls12_conn *conns;       /* master only */
    const tlsrec_tls13_secret *transcripts;
    const uint8_t *offered;               /* 16 bytes per connection, 12 compared; with match, or both NULL */
    uint8_t *verify;                      /* 16 bytes per connection; may be NULL */
    uint32_t *match;
    uint32_t count, aligned, l0, l1;      /* l0, l1: "clie" "nt f" or "serv" "er f" */
};

template <class T> __global__ void __launch_bounds__(64) tls12_finished_kernel(Tls12FinishedArgs a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8];
    /* every load is issued before the first compression */
    uint32_t Hs[T::HC], S[20], X[3], O[3] = { 0u, 0u, 0u };
    load_cells<T::HC>(a.transcripts[i].secret, (a.aligned & AL_TRANSCRIPT) != 0, Hs);
    if (a.match) load_cells<3>(a.offered + 16 * (size_t) i, (a.aligned & AL_OFFERED12) != 0, O);
    {
        uint32_t M[12];
        W kb[16];
        load_cells<12>(reinterpret_cast<const uint8_t *>(a.conns + i), (a.aligned & AL_CONNS) != 0, M);
        msg_block<T, 12, NO_PAD>(kb, M, 48, 0);
#pragma unroll
        for (int j = 0; j < 12; j++) M[j] = 0;
        hmac_mid_block<T>(kb, ip, op);
    }
    S[0] = a.l0;
    S[1] = a.l1;
    S[2] = 0x696e6973u;          /* "inis" */
    S[3] = 0x68656400u | (Hs[0] >> 24);         /* "hed" */
#pragma unroll
    for (int k = 1; k < T::HC; k++) S[3 + k] = (Hs[k - 1] << 8) | (Hs[k] >> 24);
    S[3 + T::HC] = Hs[T::HC - 1] << 8;
#pragma unroll
    for (int k = 4 + T::HC; k < 20; k++) S[k] = 0;
    tls12_p_hash<T, 15 + (int) T::HB, 3>(ip, op, S, X);
    if (a.verify) {
        uint8_t *b = a.verify + 16 * (size_t) i;
        if (a.aligned & AL_VERIFY) {
            *reinterpret_cast<uint4 *>(b) = make_uint4(__builtin_bswap32(X[0]), __builtin_bswap32(X[1]),
                                                       __builtin_bswap32(X[2]), 0u);
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t v = c < 3 ? X[c] : 0u;
                b[4 * c] = (uint8_t) (v >> 24); b[4 * c + 1] = (uint8_t) (v >> 16);
                b[4 * c + 2] = (uint8_t) (v >> 8); b[4 * c + 3] = (uint8_t) v;
            }
        }
    }
    if (a.match) {
        /* mbedtls_ct_memcmp over 12 bytes: the OR of the XOR of the three cells, no early exit, no branch on the data */
        const uint32_t d = (X[0] ^ O[0]) | (X[1] ^ O[1]) | (X[2] ^ O[2]);
        a.match[i] = d == 0 ? 1u : 0u;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) X[j] = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 20; j++) S[j] = 0;
}

} /* namespace tlsks */

using namespace tlsks;

extern "C" int tlsrec_tls12_split_key_block(int cipher, const unsigned char *keyblk, size_t keyblk_len,
                                            tlsrec_key_set *keys)
{
    if (!keys || !keyblk) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t kl = tlsrec_cipher_keylen(cipher);
    if (kl == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    const size_t il = tls12_fixed_ivlen(cipher);
    if (keyblk_len < 2 * kl + 2 * il) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    memset(keys, 0, sizeof(*keys));
    /* ssl_tls.c:7858-7892 with mac_key_len = 0: key1 = keyblk, key2 = key1 + keylen,
     * the IVs follow; the client writes with key1 / the first IV */
    memcpy(keys->client_write_key, keyblk, kl);
    memcpy(keys->server_write_key, keyblk + kl, kl);
    memcpy(keys->client_write_iv, keyblk + 2 * kl, il);
    memcpy(keys->server_write_iv, keyblk + 2 * kl + il, il);
    keys->key_len = kl;
    keys->iv_len = il;
    return 0;
}

extern "C" int tlsrec_tls12_split_key_block_cbc(int cipher, int mac, const unsigned char *keyblk, size_t keyblk_len,
                                                tlsrec_cbc_key_set *out)
{
    if (!out || !keyblk) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t kl = cbc_split_keylen(cipher), ml = cbc_split_maclen(mac);
    if (!cbc_split_pair_ok(cipher, mac)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (keyblk_len < 2 * ml + 2 * kl) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    memset(out, 0, sizeof(*out));
    tlsrec_cbc_key_material *dir[2] = { &out->client_write, &out->server_write };
    for (int i = 0; i < 2; i++) {
        dir[i]->cipher = (uint8_t) cipher;
        dir[i]->tls_minor = 3;
        dir[i]->mac = (uint8_t) mac;
        memcpy(dir[i]->mac_key, keyblk + i * ml, ml);
        memcpy(dir[i]->key, keyblk + 2 * ml + i * kl, kl);
    }
    return 0;
}

static int tls12_check(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int prf,
                       const tlsrec_tls12_conn *conns)
{
    if (!kt || (!conns && count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!keytab_range_ok(kt, first, (uint64_t) count * 2)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (tlsrec_cipher_keylen(cipher) == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (prf_index(prf) < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    return 0;
}

/* The derive kernel alone (see tlsrec__tls13_stage_keys). */
extern "C" int tlsrec__tls12_stage_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int prf,
                                        const tlsrec_tls12_conn *conns, void *stream)
{
    int r = tls12_check(kt, first, count, cipher, prf, conns);
    if (r != 0 || count == 0) return r;
    const uint32_t kl = tlsrec_cipher_keylen(cipher);
    Tls12Args a;
    a.conns = conns;
    a.out = tlsrec__keytab_stage(kt) + first;
    a.count = count;
    a.cipher = (uint32_t) cipher;
    a.taglen = tlsrec_cipher_taglen(cipher);
    a.aligned = ((uintptr_t) conns & 15) == 0;     /* 112-byte records: 16-byte loads if the array is aligned */
    hipStream_t st = (hipStream_t) stream;
    return launch_status(by_hash(prf_index(prf), [&](auto t) {
        typedef decltype(t) T;
        return cipher == TLSREC_CIPHER_CHACHA20_POLY1305 ? launch_lanes(tls12_derive_kernel<T, 32, 12>, count, st, a)
               : kl == 16 ? launch_lanes(tls12_derive_kernel<T, 16, 4>, count, st, a)
               : kl == 24 ? launch_lanes(tls12_derive_kernel<T, 24, 4>, count, st, a)
                          : launch_lanes(tls12_derive_kernel<T, 32, 4>, count, st, a);
    }));
}

extern "C" int tlsrec_tls12_keytab_derive(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int prf,
                                          const tlsrec_tls12_conn *conns, void *stream)
{
    int r = tlsrec__tls12_stage_keys(kt, first, count, cipher, prf, conns, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, 2 * count, cipher, (hipStream_t) stream);
    return r;
}

/* ---- the same for the CBC + HMAC suites ---- */
template <class T, int KL> static hipError_t tls12_launch_cbc(size_t ml, const Tls12CbcArgs &a, hipStream_t st)
{
    return ml == 20 ? launch_lanes(tls12_derive_cbc_kernel<T, KL, 20>, a.count, st, a)
           : ml == 32 ? launch_lanes(tls12_derive_cbc_kernel<T, KL, 32>, a.count, st, a)
                      : launch_lanes(tls12_derive_cbc_kernel<T, KL, 48>, a.count, st, a);
}

/* The derive kernel alone: 2 * count tlsrec_cbc_key_material records into the
 * table's CBC staging area, nothing committed (see tlsrec__tls13_stage_keys). */
extern "C" int tlsrec__tls12_stage_keys_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int mac,
                                            int etm, int prf, const tlsrec_tls12_conn *conns, void *stream)
{
    if (!kt || (!conns && count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!keytab_range_ok(kt, first, (uint64_t) count * 2)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t kl = cbc_split_keylen(cipher), ml = cbc_split_maclen(mac);
    if (!cbc_split_pair_ok(cipher, mac)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    const int alg = prf_index(prf);
    if (alg < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (etm < 0 || etm > 1) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    tlsrec_cbc_key_material *stage = tlsrec__keytab_stage_cbc(kt);
    if (!stage) return TLSREC_ERR_SSL_ALLOC_FAILED;
    Tls12CbcArgs a;
    a.conns = conns;
    a.out = stage + first;
    a.count = count;
    a.head = (uint32_t) cipher | (3u << 8) | ((uint32_t) mac << 16) | ((uint32_t) etm << 24);
    a.aligned = ((uintptr_t) conns & 15) == 0;
    hipStream_t st = (hipStream_t) stream;
    return launch_status(by_hash(alg, [&](auto t) {
        return kl == 16 ? tls12_launch_cbc<decltype(t), 16>(ml, a, st) : tls12_launch_cbc<decltype(t), 32>(ml, a, st);
    }));
}

extern "C" int tlsrec_tls12_keytab_derive_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int mac,
                                              int etm, int prf, const tlsrec_tls12_conn *conns, void *stream)
{
    int r = tlsrec__tls12_stage_keys_cbc(kt, first, count, cipher, mac, etm, prf, conns, stream);
    if (r == 0 && count)
        r = tlsrec__keytab_commit_staged_cbc(kt, first, 2 * count, cipher, mac, etm, (hipStream_t) stream);
    return r;
}

/* ---- the handshake before the key expansion: master secret, Finished ---- */
extern "C" int tlsrec_tls12_batch_compute_master(int prf, uint32_t pms_len, int extended_ms,
                                                 const tlsrec_tls12_pms_conn *conns, tlsrec_tls12_conn *out,
                                                 uint32_t count, void *stream)
{
    const int alg = prf_index(prf);
    if (alg < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if ((!conns || !out) && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (pms_len == 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (pms_len > sizeof(conns->premaster)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (count == 0) return 0;
    if (!device_ready()) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls12MasterArgs a;
    a.conns = conns;
    a.out = out;
    a.count = count;
    a.pms_len = pms_len;
    a.aligned = al(conns, AL_CONNS) | al(out, AL_AUX);     /* 240- and 112-byte records */
    hipStream_t st = (hipStream_t) stream;
    return launch_status(by_hash(alg, [&](auto t) {
        return extended_ms ? launch_lanes(tls12_master_kernel<decltype(t), true>, count, st, a)
                           : launch_lanes(tls12_master_kernel<decltype(t), false>, count, st, a);
    }));
}

extern "C" int tlsrec_tls12_batch_verify_data(int prf, int from, const tlsrec_tls12_conn *conns,
                                              const tlsrec_tls13_secret *transcripts, const uint8_t *offered,
                                              uint8_t *verify, uint32_t *match, uint32_t count, void *stream)
{
    const int alg = prf_index(prf);
    if (alg < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (from != TLSREC_IS_CLIENT && from != TLSREC_IS_SERVER) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if ((!conns || !transcripts) && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if ((offered == nullptr) != (match == nullptr)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!verify && !match && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    if (!device_ready()) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls12FinishedArgs a;
    a.conns = conns;
    a.transcripts = transcripts;
    a.offered = offered;
    a.verify = verify;
    a.match = match;
    a.count = count;
    a.aligned = al(conns, AL_CONNS) | al(transcripts, AL_TRANSCRIPT) | al(offered, AL_OFFERED12) | al(verify, AL_VERIFY);
    /* "client finished" / "server finished" (ssl_tls.c:7217-7219): the first two cells differ */
    a.l0 = from == TLSREC_IS_CLIENT ? 0x636c6965u : 0x73657276u;
    a.l1 = from == TLSREC_IS_CLIENT ? 0x6e742066u : 0x65722066u;
    return launch_status(by_hash(alg, [&](auto t) {
        return launch_lanes(tls12_finished_kernel<decltype(t)>, count, (hipStream_t) stream, a);
    }));
}

