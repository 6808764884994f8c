/*
 * exporter.hip -- keying-material exporters in batches (RFC 8446 7.5, RFC
 * 5705), one connection per lane, on the word-wise blocks of tlsrec_kdf.h:
 *
 *   reference                                             here
 *   mbedtls_ssl_tls13_exporter  (ssl_tls13_keys.c:1828)   tlsrec_tls13_batch_exporter
 *   mbedtls_ssl_tls12_export_keying_material
 *                                    (ssl_tls.c:8886)     tlsrec_tls12_batch_export_keying_material
 *
 * The single-shot forms (tlsrec_tls13_exporter,
 * tlsrec_tls12_export_keying_material) are in keysched.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_internal.h"
#include "tlsrec_kdf.h"

namespace tlsks {

/* ---- keying material exporters (RFC 8446 7.5, RFC 5705) ---------------------
 * mbedtls_ssl_tls13_exporter (ssl_tls13_keys.c:1828-1858) and
 * mbedtls_ssl_tls12_export_keying_material (ssl_tls.c:8886-8936), one connection
 * per lane.  Unlike the rest of the family the shapes are
 * not fixed: the label (up to 249 bytes), the context (up to 255) and the output
 * (up to 8160) are run-time values, the same for every lane of a call, so the
 * loops over their blocks are rolled and their trip counts are scalar.
 *
 * What is the same for every connection is built on the host: in TLS 1.3 the
 * whole padded inner message of the first Expand-Label (exporter_blocks(), a
 * kernel argument) and the "exporter" HkdfLabel prefix.  What is per connection
 * and public -- the context, the randoms, the assembled PRF seed -- is staged in
 * LDS as big-endian cells, cell g of lane l at pub[g * 64 + l]: a wave's access
 * to one cell falls in 64 different banks, a rolled loop can index it, and a
 * lane touches its own column only, so there is no barrier.  What is secret
 * (the exporter secret, the master secret, every midstate, S1, A(i), T(k)) is in
 * registers only; each output block is stored as soon as it is made.
 *
 * Compressions per connection (exporters), with b(n) = ceil((n + 1 + LENB) / BB),
 * iters = ceil(out_len / H), L the label's length, C the context's:
 *   TLS 1.3: 2 + (b(11 + L + H) + 1) + 2 + (C ? b(C) : 0) + 2 + 3 (iters - 1)
 *   TLS 1.2, N = L + 64 (+ 2 + C): 2 + (b(N) + 1) + iters (b(H + N) + 1) + 2 (iters - 1) */
enum { EXP13_CELLS = 64, EXP12_CELLS = 160 };

/* byte p of the lane's column */
__device__ __forceinline__ void pub_put(uint32_t *pub, uint32_t p, uint32_t byte)
{
    reinterpret_cast<uint8_t *>(pub + (p >> 2) * 64 + threadIdx.x)[3 - (p & 3)] = (uint8_t) byte;
}

/* 0x80 after a message of n bytes, and zeros to the end of its cell */
__device__ __forceinline__ void pub_close(uint32_t *pub, uint32_t n)
{
    pub_put(pub, n, 0x80);
    for (uint32_t p = n + 1; p & 3; p++) pub_put(pub, p, 0);
}

/* One block of a padded message out of the lane's column: cells FROM.. of the
 * block that starts at cell `first`; cells from `lim` on are zero, and `bits`
 * closes the block when it is the last.  Cells below FROM are left zero for the
 * caller.  first, lim and last are wave-uniform. */
template <class T, int FROM, int CELLS>
__device__ __forceinline__ void pub_block(typename T::W (&w)[16], const uint32_t *pub, uint32_t first, uint32_t lim,
                                          bool last, uint32_t bits)
{
    constexpr int CPB = T::BB / 4;
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (int c = FROM; c < CPB; c++) {
        const uint32_t g = first + c;
        const uint32_t v = pub[(g < CELLS ? g : CELLS - 1) * 64 + threadIdx.x];
        or_cell<T>(w, c, g < lim ? v : 0u);
    }
    if (last) w[15] = (typename T::W) bits;
}

/* `take` (1..H, wave-uniform) bytes of x to dst: 16-byte stores for the whole groups if al16, bytes otherwise */
template <class T>
__device__ __forceinline__ void store_out(uint8_t *dst, bool al16, const typename T::W (&x)[T::HW], uint32_t take)
{
#pragma unroll
    for (int g = 0; g < T::HB / 16; g++) {
        uint32_t m[4];
#pragma unroll
        for (int j = 0; j < 4; j++) m[j] = __builtin_bswap32(cell<T, T::HW>(x, 4 * g + j));
        if (al16 && take >= 16u * g + 16u) {
            *reinterpret_cast<uint4 *>(dst + 16 * g) = make_uint4(m[0], m[1], m[2], m[3]);
        } else {
#pragma unroll
            for (int b = 0; b < 16; b++)
                if (16u * g + b < take) dst[16 * g + b] = (uint8_t) (m[b >> 2] >> (8 * (b & 3)));
        }
#pragma unroll
        for (int j = 0; j < 4; j++) m[j] = 0;
    }
}

enum { OFF_EXPORTER = 18, AL_OUT = AL_AUX, AL_SECRETS = AL_MASTER };

template <class T> struct Tls13ExporterArgs {
    const tlsrec_tls13_secret *secrets;
    const uint8_t *contexts;
    uint8_t *out;
    uint32_t count, context_len, context_stride, out_len, out_stride, aligned, nblk;
    LabelW label;                          /* HkdfLabel(out_len, "exporter", a context of H bytes) */
    typename T::W empty[T::HW];            /* Hash("") */
    typename T::W words[T::BB == 64 ? 80 : 48];   /* HkdfLabel(H, label, Hash("")) || 0x01, padded: nblk blocks */
};

template <class T> __global__ void __launch_bounds__(64) tls13_exporter_kernel(Tls13ExporterArgs<T> a)
{
    typedef typename T::W W;
    constexpr int CPB = T::BB / 4;
    constexpr int EC = 5 + T::HC, NC = T::HC + EC, LK = 2 * T::HB + OFF_EXPORTER + 1;
    static_assert(LK + 1 + T::LENB > T::BB && LK + 1 + T::LENB <= 2 * T::BB, "T(k > 1) takes two inner blocks");
    __shared__ uint32_t pub[EXP13_CELLS * 64];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8], w[16], st[8], x[T::HW], hc[T::HW];
    load_digest<T>(a.secrets[i].secret, (a.aligned & AL_SECRETS) != 0, x);
    const uint32_t n = a.context_len;
    if (n) {
        const uint8_t *c = a.contexts + (size_t) i * a.context_stride;
#pragma unroll 1
        for (uint32_t p = 0; p < n; p++) pub_put(pub, p, c[p]);
        pub_close(pub, n);
    }
    /* S1 = Expand-Label(secret, label, Hash(""), H): the same inner message for every lane */
    hmac_mid<T>(x, ip, op);
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = ip[j];
#pragma unroll 1
    for (uint32_t b = 0; b < a.nblk; b++) {
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = a.words[16 * b + j];
        sha_compress<typename T::S>(st, w);
    }
    hmac_outer<T>(op, st, x);
    hmac_mid<T>(x, ip, op);
    /* Hash(context) */
    if (n) {
        const uint32_t nb = (n + 1 + T::LENB + T::BB - 1) / T::BB, lim = (n + 4) / 4;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = T::iv(j);
#pragma unroll 1
        for (uint32_t b = 0; b < nb; b++) {
            pub_block<T, 0, EXP13_CELLS>(w, pub, b * CPB, lim, b + 1 == nb, n * 8);
            sha_compress<typename T::S>(st, w);
        }
#pragma unroll
        for (int j = 0; j < T::HW; j++) hc[j] = st[j];
    } else {
#pragma unroll
        for (int j = 0; j < T::HW; j++) hc[j] = a.empty[j];
    }
    /* T(1) = HMAC(S1, HkdfLabel || 0x01): one inner block */
    uint8_t *dst = a.out + (size_t) i * a.out_stride;
    const bool oal = (a.aligned & AL_OUT) != 0;
    uint32_t left = a.out_len;
    label_block<T, OFF_EXPORTER, true>(w, a.label, hc);
    hmac_block<T>(ip, op, w, x);
    store_out<T>(dst, oal, x, left < T::HB ? left : (uint32_t) T::HB);
    /* T(k) = HMAC(S1, T(k - 1) || HkdfLabel || k): H + 18 + H + 1 bytes, two inner blocks */
    uint32_t E[EC];
#pragma unroll
    for (int c = 0; c < 4; c++) E[c] = a.label.c[c];
    E[4] = a.label.c[4] | (cell<T, T::HW>(hc, 0) >> 16);
#pragma unroll
    for (int k = 1; k < T::HC; k++) E[4 + k] = (cell<T, T::HW>(hc, k - 1) << 16) | (cell<T, T::HW>(hc, k) >> 16);
    E[4 + T::HC] = cell<T, T::HW>(hc, T::HC - 1) << 16;
#pragma unroll 1
    for (uint32_t k = 2; left > T::HB; k++) {
        left -= T::HB;
        dst += T::HB;
        uint32_t M[NC];
#pragma unroll
        for (int c = 0; c < T::HC; c++) M[c] = cell<T, T::HW>(x, c);
#pragma unroll
        for (int c = 0; c < EC; c++) M[T::HC + c] = E[c];
        M[NC - 1] |= k << 8;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        msg_block<T, NC>(w, M, LK, 0);
        sha_compress<typename T::S>(st, w);
        msg_block<T, NC>(w, M, LK, 1);
        sha_compress<typename T::S>(st, w);
        hmac_outer<T>(op, st, x);
        store_out<T>(dst, oal, x, left < T::HB ? left : (uint32_t) T::HB);
#pragma unroll
        for (int c = 0; c < T::HC; c++) M[c] = 0;
    }
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; hc[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; st[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

struct Tls12ExportArgs {
    const tlsrec_tls12_conn *conns;
    const uint8_t *contexts;
    uint8_t *out;
    uint32_t count, label_len, context_len, context_stride, use_context, out_len, out_stride, aligned;
    uint32_t label[63];                   /* big-endian cells, zero-padded */
};

/* P_hash(master, S) with S = label || client_random || server_random
 * [|| uint16(context_len) || context], N bytes, staged from cell HC of the lane's
 * column on: the inner message of A(1) is S, that of an output block is A(i) || S,
 * whose first HC cells come from registers and whose rest is the same column read
 * from cell HC on. */
template <class T> __global__ void __launch_bounds__(64) tls12_export_kernel(Tls12ExportArgs a)
{
    typedef typename T::W W;
    constexpr int CPB = T::BB / 4;
    constexpr uint32_t S0 = 4 * T::HC;    /* the byte of the column at which S starts */
    __shared__ uint32_t pub[EXP12_CELLS * 64];
    static_assert(T::HC + (249 + 64 + 2 + 255 + 4) / 4 <= EXP12_CELLS, "the longest seed fits the column");
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint8_t *conn = reinterpret_cast<const uint8_t *>(a.conns + i);
    const bool cal = (a.aligned & AL_CONNS) != 0;
    W ip[8], op[8], w[16], st[8], A[T::HW], D[T::HW];
    uint32_t R[16];
    load_cells<16>(conn + 48, cal, R);
    {
        uint32_t M[12];
        W kb[16];
        load_cells<12>(conn, cal, M);
        msg_block<T, 12, NO_PAD>(kb, M, 48, 0);
#pragma unroll
        for (int j = 0; j < 12; j++) M[j] = 0;
        hmac_mid_block<T>(kb, ip, op);
    }
    /* the seed: the label by cells, then bytes */
#pragma unroll 1
    for (uint32_t c = 0; 4 * c < a.label_len; c++) pub[(T::HC + c) * 64 + threadIdx.x] = a.label[c];
    uint32_t p = S0 + a.label_len;
    /* randbytes is server_random || client_random: client_random goes first (ssl_tls.c:8920-8925) */
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t v = R[(k + 8) & 15];
#pragma unroll
        for (int j = 0; j < 4; j++) pub_put(pub, p + 4 * k + j, v >> (24 - 8 * j));
    }
    p += 64;
    if (a.use_context) {
        pub_put(pub, p, a.context_len >> 8);
        pub_put(pub, p + 1, a.context_len);
        p += 2;
        const uint8_t *c = a.contexts + (size_t) i * a.context_stride;
#pragma unroll 1
        for (uint32_t q = 0; q < a.context_len; q++) pub_put(pub, p + q, c[q]);
        p += a.context_len;
    }
    pub_close(pub, p);
    const uint32_t N = p - S0, lim = (p + 4) / 4;
    /* A(1) = HMAC(master, S) */
    {
        const uint32_t nb = (N + 1 + T::LENB + T::BB - 1) / T::BB;
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
#pragma unroll 1
        for (uint32_t b = 0; b < nb; b++) {
            pub_block<T, 0, EXP12_CELLS>(w, pub, T::HC + b * CPB, lim, b + 1 == nb, (T::BB + N) * 8);
            sha_compress<typename T::S>(st, w);
        }
        hmac_outer<T>(op, st, A);
    }
    uint8_t *dst = a.out + (size_t) i * a.out_stride;
    const bool oal = (a.aligned & AL_OUT) != 0;
    const uint32_t nb = (T::HB + N + 1 + T::LENB + T::BB - 1) / T::BB, bits = (T::BB + T::HB + N) * 8;
    uint32_t left = a.out_len;
#pragma unroll 1
    for (;;) {
        /* output block = HMAC(master, A(i) || S) */
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        pub_block<T, T::HC, EXP12_CELLS>(w, pub, 0, lim, nb == 1, bits);
#pragma unroll
        for (int c = 0; c < T::HC; c++) or_cell<T>(w, c, cell<T, T::HW>(A, c));
        sha_compress<typename T::S>(st, w);
#pragma unroll 1
        for (uint32_t b = 1; b < nb; b++) {
            pub_block<T, 0, EXP12_CELLS>(w, pub, b * CPB, lim, b + 1 == nb, bits);
            sha_compress<typename T::S>(st, w);
        }
        hmac_outer<T>(op, st, D);
        store_out<T>(dst, oal, D, left < T::HB ? left : (uint32_t) T::HB);
        if (left <= T::HB) break;
        left -= T::HB;
        dst += T::HB;
        /* A(i + 1) = HMAC(master, A(i)) */
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        digest_block<T>(w, A);
        sha_compress<typename T::S>(st, w);
        hmac_outer<T>(op, st, A);
    }
#pragma unroll
    for (int j = 0; j < T::HW; j++) { A[j] = 0; D[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; st[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

} /* namespace tlsks */

using namespace tlsks;

/* Host-only: the inner message of the exporter's first step (ssl_tls13_keys.c:1838),
 * HkdfLabel(H, label, Hash("")) || 0x01, the same for every connection of a call:
 * 11 + label_len + H bytes, padded as the blocks after an HMAC's ipad block (0x80,
 * zeros, the length (BB + n) * 8) into big-endian words widened to 64 bits, 16 a
 * block; *nblk blocks, at most 5 (SHA-256) or 3 (SHA-384).  words_out holds 80. */
extern "C" int tlsrec__tls13_exporter_blocks(int hash_alg, const unsigned char *label, size_t label_len,
                                             uint64_t *words_out, uint32_t *nblk)
{
    const int a = alg_index(hash_alg);
    if (a < 0 || !words_out || !nblk || (!label && label_len) || label_len > MAX_LABEL)
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t H = alg_len(a), BB = a == H_SHA384 ? 128 : 64, LENB = BB / 8, wb = BB / 16;
    uint8_t e[48], m[5 * 64 + 128] = { 0 };
    for (size_t j = 0; j < H; j++) {
        e[j] = a == H_SHA384 ? (uint8_t) (ladder_consts<L384>().empty[j / 8] >> (56 - 8 * (j % 8)))
                             : (uint8_t) (ladder_consts<L256>().empty[j / 4] >> (24 - 8 * (j % 4)));
    }
    size_t n = encode_label(H, label, label_len, e, H, m);
    m[n++] = 0x01;
    const size_t blocks = (n + 1 + LENB + BB - 1) / BB;
    const uint64_t bits = (uint64_t) (BB + n) * 8;
    m[n] = 0x80;
    for (size_t j = 0; j < 8; j++) m[blocks * BB - 1 - j] = (uint8_t) (bits >> (8 * j));
    for (size_t k = 0; k < 16 * blocks; k++) {
        uint64_t v = 0;
        for (size_t j = 0; j < wb; j++) v = (v << 8) | m[k * wb + j];
        words_out[k] = v;
    }
    *nblk = (uint32_t) blocks;
    return 0;
}

/* ---- keying material exporters in batches (tls13_exporter_kernel, tls12_export_kernel) ---- */
static const uint32_t EXPORT_MAX_KEY_LEN = 8160;     /* MBEDTLS_SSL_EXPORT_MAX_KEY_LEN, ssl.h */
static const uint32_t EXPORT_MAX_CONTEXT = 255;      /* the batch form's limit: longer contexts stay single-shot */

/* the checks the two exporter batches share, in the header's order, after the hash / PRF; `ctx`: a context is used */
static int export_check(const void *in, const void *contexts, const void *out, const void *label, size_t label_len,
                        bool ctx, uint32_t context_len, uint32_t context_stride, uint32_t out_len, uint32_t out_stride,
                        uint32_t count)
{
    if (count && (!in || !out || (!contexts && ctx && context_len))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!label && label_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (label_len > MAX_LABEL) return TLSREC_ERR_SSL_BAD_INPUT_DATA;                      /* ssl_tls.c:8959 */
    if (out_len > EXPORT_MAX_KEY_LEN) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (out_stride < out_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (ctx && context_stride != 0 && context_stride < context_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (ctx && context_len > EXPORT_MAX_CONTEXT) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    return 0;
}

template <class T>
static hipError_t exporter_launch(const tlsrec_tls13_secret *secrets, const unsigned char *label, size_t label_len,
                                  const uint8_t *contexts, uint32_t context_len, uint32_t context_stride, uint8_t *out,
                                  uint32_t out_len, uint32_t out_stride, uint32_t count, int hash_alg, hipStream_t st)
{
    Tls13ExporterArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.secrets = secrets;
    a.contexts = contexts;
    a.out = out;
    a.count = count;
    a.context_len = context_len;
    a.context_stride = context_stride;
    a.out_len = out_len;
    a.out_stride = out_stride;
    a.aligned = al(secrets, AL_SECRETS) | al_out(out, out_stride);
    a.label = label_cells(out_len, "exporter", 8, T::HB);
    for (int j = 0; j < T::HW; j++) a.empty[j] = ladder_consts<T>().empty[j];
    uint64_t words[80];
    if (tlsrec__tls13_exporter_blocks(hash_alg, label, label_len, words, &a.nblk) != 0) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < 16 * a.nblk; k++) a.words[k] = (typename T::W) words[k];
    return launch_lanes(tls13_exporter_kernel<T>, count, st, a);
}

extern "C" int tlsrec_tls13_batch_exporter(int hash_alg, const tlsrec_tls13_secret *secrets,
                                           const unsigned char *label, size_t label_len, const uint8_t *contexts,
                                           uint32_t context_len, uint32_t context_stride, uint8_t *out,
                                           uint32_t out_len, uint32_t out_stride, uint32_t count, void *stream)
{
    const int alg = alg_index(hash_alg);
    if (alg < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const int r = export_check(secrets, contexts, out, label, label_len, true, context_len, context_stride, out_len,
                               out_stride, count);
    if (r != 0 || count == 0 || out_len == 0) return r;
    if (!device_ready()) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    return launch_status(by_hash(alg, [&](auto t) {
        return exporter_launch<decltype(t)>(secrets, label, label_len, contexts, context_len, context_stride, out, out_len,
                                            out_stride, count, hash_alg, (hipStream_t) stream);
    }));
}

extern "C" int tlsrec_tls12_batch_export_keying_material(int prf, const tlsrec_tls12_conn *conns, const char *label,
                                                         size_t label_len, const uint8_t *contexts,
                                                         uint32_t context_len, uint32_t context_stride,
                                                         int use_context, uint8_t *out, uint32_t out_len,
                                                         uint32_t out_stride, uint32_t count, void *stream)
{
    const int alg = prf_index(prf);
    if (alg < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const int r = export_check(conns, contexts, out, label, label_len, use_context != 0, context_len, context_stride,
                               out_len, out_stride, count);
    if (r != 0 || count == 0 || out_len == 0) return r;
    if (!device_ready()) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls12ExportArgs a;
    memset(&a, 0, sizeof(a));
    a.conns = conns;
    a.contexts = contexts;
    a.out = out;
    a.count = count;
    a.label_len = (uint32_t) label_len;
    a.use_context = use_context != 0;
    a.context_len = use_context ? context_len : 0;
    a.context_stride = use_context ? context_stride : 0;
    a.out_len = out_len;
    a.out_stride = out_stride;
    a.aligned = al(conns, AL_CONNS) | al_out(out, out_stride);
    for (size_t k = 0; k < label_len; k++) a.label[k >> 2] |= (uint32_t) (unsigned char) label[k] << (24 - 8 * (k & 3));
    return launch_status(by_hash(alg, [&](auto t) {
        return launch_lanes(tls12_export_kernel<decltype(t)>, count, (hipStream_t) stream, a);
    }));
}

