/*
 * keysched.hip -- the single-shot key-schedule calls on the GPU (SURVEY.md
 * 8(f)-3): a byte-wise SHA-2 / HMAC / HKDF-Expand / TLS 1.2 PRF of any shape,
 * run as a short chain of jobs out of a small device arena.
 *
 * HKDF-SHA256 / HKDF-SHA384 (RFC 5869 over FIPS 180-4, HMAC per RFC 2104)
 * with the TLS 1.3 label encoding of library/ssl_tls13_keys.c:
 *
 *   reference                                   here
 *   ssl_tls13_hkdf_encode_label      :98-136    encode_label()       (tlsrec_kdf.h; host: framing only)
 *   mbedtls_ssl_tls13_hkdf_expand_label :138    tlsrec_tls13_hkdf_expand_label
 *   mbedtls_ssl_tls13_make_traffic_keys :262    tlsrec_tls13_make_traffic_keys
 *   mbedtls_ssl_tls13_derive_secret     :293    tlsrec_tls13_derive_secret
 *   mbedtls_ssl_tls13_evolve_secret     :332    tlsrec_tls13_evolve_secret
 *   mbedtls_ssl_tls13_exporter          :1828   tlsrec_tls13_exporter
 *   "traffic upd" (ssl_tls13_keys.h:16)         tlsrec_tls13_update_traffic_secret (RFC 8446 7.2)
 *   (batch)                                     tlsrec_tls13_keytab_derive: secrets in HBM ->
 *                                               key material -> key-table slots, no host round trip
 *   ..._derive_early / _handshake / _application_secrets,
 *   ..._derive_resumption_master_secret :421-650 tlsrec_tls13_derive_*_secrets, ..._resumption_master_secret
 *   ssl_tls13_calc_finished_core        :697    tlsrec_tls13_calc_finished
 *   mbedtls_ssl_tls13_create_psk_binder :832    tlsrec_tls13_create_psk_binder
 *
 * Every hash, HMAC and HKDF step runs in a kernel; the host only encodes the
 * HkdfLabel byte string (length, "tls13 " + label, context length), moves
 * bytes and checks arguments the way the reference does.  One thread per
 * derivation: this is per-connection control work (a few SHA compressions),
 * not the bulk path, so lanes are independent and the message buffers live
 * in per-lane scratch.
 *
 * Also the single-shot TLS 1.2 / DTLS 1.2 calls of library/ssl_tls.c (the PRF
 * of RFC 5246 section 5; table at the host section below) as one more job of
 * the same kernel.  The batches, whose kernels are written for their fixed
 * shapes on the word-wise blocks of tlsrec_kdf.h, are in tls13_ladder.hip,
 * tls12_batch.hip, exporter.hip and cookie.hip.
 */
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_frame.h"     /* tlsrec_cipher_keylen, tlsrec_cipher_taglen */
#include "tlsrec_internal.h"
#include "tlsrec_kdf.h"      /* H_SHA256 / H_SHA384, encode_label, the key-block shapes; tlsrec_sha.h: kK256 / kK512, ror32 / ror64 */

namespace tlsks {

/* The message block is kept as big-endian words (16 x 32 bit for SHA-256,
 * 16 x 64 bit for SHA-384), filled a byte at a time. */
struct Hash {
    uint32_t alg;
    uint32_t fill;            /* bytes in the current block */
    uint64_t total;           /* message bytes absorbed */
    uint64_t st[8];           /* SHA-256 uses the low 32 bits */
    uint64_t w[16];           /* SHA-256 uses the low 32 bits of w[0..15] */
};

__device__ __forceinline__ uint32_t blk_bytes(uint32_t alg) { return alg == H_SHA384 ? 128u : 64u; }
__device__ __forceinline__ uint32_t out_bytes(uint32_t alg) { return alg == H_SHA384 ? 48u : 32u; }

__device__ void compress(Hash &h)
{
    if (h.alg == H_SHA384) {
        uint64_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = h.w[i];
        uint64_t a = h.st[0], b = h.st[1], c = h.st[2], d = h.st[3], e = h.st[4], f = h.st[5], g = h.st[6],
                 k = h.st[7];
        for (int i = 0; i < 80; i++) {
            uint64_t wi;
            if (i < 16) {
                wi = w[i & 15];
            } else {
                const uint64_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
                wi = w[i & 15] + (ror64(w15, 1) ^ ror64(w15, 8) ^ (w15 >> 7)) + w[(i - 7) & 15] +
                     (ror64(w2, 19) ^ ror64(w2, 61) ^ (w2 >> 6));
                w[i & 15] = wi;
            }
            const uint64_t t1 = k + (ror64(e, 14) ^ ror64(e, 18) ^ ror64(e, 41)) + ((e & f) ^ (~e & g)) + kK512[i] + wi;
            const uint64_t t2 = (ror64(a, 28) ^ ror64(a, 34) ^ ror64(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
            k = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h.st[0] += a; h.st[1] += b; h.st[2] += c; h.st[3] += d;
        h.st[4] += e; h.st[5] += f; h.st[6] += g; h.st[7] += k;
    } else {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = (uint32_t) h.w[i];
        uint32_t a = (uint32_t) h.st[0], b = (uint32_t) h.st[1], c = (uint32_t) h.st[2], d = (uint32_t) h.st[3];
        uint32_t e = (uint32_t) h.st[4], f = (uint32_t) h.st[5], g = (uint32_t) h.st[6], k = (uint32_t) h.st[7];
        for (int i = 0; i < 64; i++) {
            uint32_t wi;
            if (i < 16) {
                wi = w[i & 15];
            } else {
                const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
                wi = w[i & 15] + (ror32(w15, 7) ^ ror32(w15, 18) ^ (w15 >> 3)) + w[(i - 7) & 15] +
                     (ror32(w2, 17) ^ ror32(w2, 19) ^ (w2 >> 10));
                w[i & 15] = wi;
            }
            const uint32_t t1 = k + (ror32(e, 6) ^ ror32(e, 11) ^ ror32(e, 25)) + ((e & f) ^ (~e & g)) + kK256[i] + wi;
            const uint32_t t2 = (ror32(a, 2) ^ ror32(a, 13) ^ ror32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            k = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h.st[0] = (uint32_t) (h.st[0] + a); h.st[1] = (uint32_t) (h.st[1] + b);
        h.st[2] = (uint32_t) (h.st[2] + c); h.st[3] = (uint32_t) (h.st[3] + d);
        h.st[4] = (uint32_t) (h.st[4] + e); h.st[5] = (uint32_t) (h.st[5] + f);
        h.st[6] = (uint32_t) (h.st[6] + g); h.st[7] = (uint32_t) (h.st[7] + k);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) h.w[i] = 0;
    h.fill = 0;
}

__device__ void hinit(Hash &h, uint32_t alg)
{
    /* FIPS 180-4 5.3.3 (SHA-256) and 5.3.4 (SHA-384) */
    const uint64_t iv256[8] = { 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19 };
    const uint64_t iv384[8] = { 0xcbbb9d5dc1059ed8ULL, 0x629a292a367cd507ULL, 0x9159015a3070dd17ULL,
                                0x152fecd8f70e5939ULL, 0x67332667ffc00b31ULL, 0x8eb44a8768581511ULL,
                                0xdb0c2e0d64f98fa7ULL, 0x47b5481dbefa4fa4ULL };
    h.alg = alg;
    h.fill = 0;
    h.total = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) h.st[i] = alg == H_SHA384 ? iv384[i] : iv256[i];
#pragma unroll
    for (int i = 0; i < 16; i++) h.w[i] = 0;
}

/* absorb one byte (no length accounting) */
__device__ __forceinline__ void put(Hash &h, uint32_t byte)
{
    const uint32_t wb = h.alg == H_SHA384 ? 8u : 4u;
    const uint32_t idx = h.fill / wb, sh = 8 * (wb - 1 - h.fill % wb);
    h.w[idx] |= (uint64_t) (byte & 0xff) << sh;
    if (++h.fill == blk_bytes(h.alg)) compress(h);
}

__device__ void update(Hash &h, const uint8_t *p, uint32_t n, uint8_t x = 0)
{
    for (uint32_t i = 0; i < n; i++) put(h, p[i] ^ x);
    h.total += n;
}

/* n copies of byte b (key padding) */
__device__ void update_fill(Hash &h, uint8_t b, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) put(h, b);
    h.total += n;
}

__device__ void finish(Hash &h, uint8_t *out)
{
    const uint64_t bits = h.total * 8;
    const uint32_t B = blk_bytes(h.alg), L = h.alg == H_SHA384 ? 16u : 8u;
    put(h, 0x80);
    while (h.fill != B - L) put(h, 0);
    for (uint32_t i = 0; i < L; i++) put(h, i < L - 8 ? 0u : (uint32_t) (bits >> (8 * (L - 1 - i))));
    const uint32_t n = out_bytes(h.alg);
    for (uint32_t i = 0; i < n; i++) {
        if (h.alg == H_SHA384) out[i] = (uint8_t) (h.st[i / 8] >> (56 - 8 * (i % 8)));
        else out[i] = (uint8_t) (h.st[i / 4] >> (24 - 8 * (i % 4)));
    }
}

/* HMAC (RFC 2104) with a key already reduced to <= one block. */
struct Hmac {
    Hash in;
    uint8_t k0[128];
    uint32_t klen;
};

__device__ void hmac_start(Hmac &m, uint32_t alg, const uint8_t *key, uint32_t klen)
{
    const uint32_t B = blk_bytes(alg);
    if (klen > B) {                     /* RFC 2104 2: hash keys longer than the block */
        Hash t;
        hinit(t, alg);
        update(t, key, klen);
        finish(t, m.k0);
        klen = out_bytes(alg);
    } else {
        for (uint32_t i = 0; i < klen; i++) m.k0[i] = key[i];
    }
    m.klen = klen;
    hinit(m.in, alg);
    update(m.in, m.k0, klen, 0x36);
    update_fill(m.in, 0x36, B - klen);
}

__device__ void hmac_end(Hmac &m, uint8_t *out)
{
    uint8_t inner[64];
    finish(m.in, inner);
    const uint32_t alg = m.in.alg, B = blk_bytes(alg);
    Hash o;
    hinit(o, alg);
    update(o, m.k0, m.klen, 0x5c);
    update_fill(o, 0x5c, B - m.klen);
    update(o, inner, out_bytes(alg));
    finish(o, out);
}

/* HKDF-Expand (RFC 5869 2.3) with info = info1 || info2:
 * T(i) = HMAC(PRK, T(i-1) || info || i), OKM = first L bytes of T(1)||T(2)... */
__device__ void hkdf_expand(uint32_t alg, const uint8_t *prk, uint32_t prk_len, const uint8_t *info1,
                            uint32_t len1, const uint8_t *info2, uint32_t len2, uint8_t *out, uint32_t out_len)
{
    const uint32_t H = out_bytes(alg);
    uint8_t t[64];
    uint32_t done = 0;
    for (uint32_t i = 1; done < out_len; i++) {
        Hmac m;
        hmac_start(m, alg, prk, prk_len);
        if (i > 1) update(m.in, t, H);
        update(m.in, info1, len1);
        update(m.in, info2, len2);
        const uint8_t ctr = (uint8_t) i;
        update(m.in, &ctr, 1);
        hmac_end(m, t);
        const uint32_t take = out_len - done < H ? out_len - done : H;
        for (uint32_t j = 0; j < take; j++) out[done + j] = t[j];
        done += take;
    }
}

/* TLS 1.2 PRF (RFC 5246 5, tls_prf_generic ssl_tls.c:6099) with seed = label || random:
 * A(0) = seed, A(i) = HMAC(secret, A(i-1)), out = HMAC(secret, A(1) || seed) || HMAC(secret, A(2) || seed) ... */
__device__ void tls_prf(uint32_t alg, const uint8_t *secret, uint32_t slen, const uint8_t *label, uint32_t llen,
                        const uint8_t *rnd, uint32_t rlen, uint8_t *out, uint32_t out_len)
{
    const uint32_t H = out_bytes(alg);
    uint8_t a[48], t[48];
    {
        Hmac m;
        hmac_start(m, alg, secret, slen);
        update(m.in, label, llen);
        update(m.in, rnd, rlen);
        hmac_end(m, a);
    }
    uint32_t done = 0;
    while (done < out_len) {
        Hmac m;
        hmac_start(m, alg, secret, slen);
        update(m.in, a, H);
        update(m.in, label, llen);
        update(m.in, rnd, rlen);
        hmac_end(m, t);
        const uint32_t take = out_len - done < H ? out_len - done : H;
        for (uint32_t j = 0; j < take; j++) out[done + j] = t[j];
        done += take;
        if (done < out_len) {
            Hmac n;
            hmac_start(n, alg, secret, slen);
            update(n.in, a, H);
            hmac_end(n, a);
        }
    }
}

/* ---------------- kernels ---------------------------------------------- */
enum { OP_HASH = 0, OP_HMAC = 1, OP_EXPAND = 2, OP_PRF = 3 };

struct Job {
    uint32_t op, alg;
    const uint8_t *key;
    uint32_t key_len;
    const uint8_t *msg;       /* message / info (first part) */
    uint32_t msg_len;
    const uint8_t *msg2;      /* info, second part (a context computed on the device) */
    uint32_t msg2_len;
    uint8_t *out;
    uint32_t out_len;
};

__global__ void __launch_bounds__(64) kdf_job_kernel(const Job *jobs, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Job j = jobs[i];
    if (j.op == OP_HASH) {
        Hash h;
        hinit(h, j.alg);
        update(h, j.msg, j.msg_len);
        update(h, j.msg2, j.msg2_len);
        finish(h, j.out);
    } else if (j.op == OP_HMAC) {
        Hmac m;
        hmac_start(m, j.alg, j.key, j.key_len);
        update(m.in, j.msg, j.msg_len);
        update(m.in, j.msg2, j.msg2_len);
        hmac_end(m, j.out);
    } else if (j.op == OP_PRF) {
        tls_prf(j.alg, j.key, j.key_len, j.msg, j.msg_len, j.msg2, j.msg2_len, j.out, j.out_len);
    } else {
        hkdf_expand(j.alg, j.key, j.key_len, j.msg, j.msg_len, j.msg2, j.msg2_len, j.out, j.out_len);
    }
}

/* Batch traffic-key derivation: one thread per connection direction.
 * infos = HkdfLabel("traffic upd", "", H) || HkdfLabel("key", "", key_len)
 *         || HkdfLabel("iv", "", 12), encoded on the host (same for all). */
struct DeriveArgs {
    tlsrec_tls13_secret *secrets;
    tlsrec_key_material *out;
    uint8_t infos[96];        /* the three encoded HkdfLabels, by value (no host staging buffer) */
    uint32_t len_upd, len_key, len_iv;
    uint32_t count, alg, cipher, key_len, update;
};

__global__ void __launch_bounds__(64) tls13_derive_kernel(DeriveArgs a)
{
    /* the encoded labels (kernel argument) staged once per workgroup */
    __shared__ uint8_t infos[96];
    for (int k = threadIdx.x; k < 96; k += blockDim.x) infos[k] = a.infos[k];
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint32_t H = out_bytes(a.alg);
    uint8_t s[48];
    for (uint32_t k = 0; k < H; k++) s[k] = a.secrets[i].secret[k];
    if (a.update) {
        /* RFC 8446 7.2: secret_N+1 = HKDF-Expand-Label(secret_N, "traffic upd", "", H) */
        uint8_t nx[48];
        hkdf_expand(a.alg, s, H, infos, a.len_upd, nullptr, 0, nx, H);
        for (uint32_t k = 0; k < H; k++) {
            s[k] = nx[k];
            a.secrets[i].secret[k] = nx[k];
        }
    }
    tlsrec_key_material km;
    uint8_t *raw = (uint8_t *) &km;
    for (int k = 0; k < 64; k++) raw[k] = 0;
    km.cipher = (uint8_t) a.cipher;
    km.tls_minor = 4;
    km.fixed_ivlen = 12;      /* TLS 1.3: fixed_ivlen = ivlen = 12, ssl_tls13_keys.c:985-998 */
    km.taglen = (uint8_t) tlsrec_cipher_taglen((int) a.cipher);
    /* ssl_tls13_make_traffic_key, ssl_tls13_keys.c:219-246 */
    hkdf_expand(a.alg, s, H, infos + a.len_upd, a.len_key, nullptr, 0, km.key, a.key_len);
    hkdf_expand(a.alg, s, H, infos + a.len_upd + a.len_key, a.len_iv, nullptr, 0, km.iv, 12);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + i);
    const uint4 *src = reinterpret_cast<const uint4 *>(&km);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = src[k];
}

} /* namespace tlsks */

using namespace tlsks;

/* ======================================================================
 * host side
 * ==================================================================== */
static const size_t MAX_CONTEXT = 64;       /* MBEDTLS_SSL_TLS1_3_KEY_SCHEDULE_MAX_CONTEXT_LEN = PSA_HASH_MAX_SIZE */
static const size_t MAX_EXPANSION = 255 * 64;   /* ..._MAX_EXPANSION_LEN = 255 * MBEDTLS_TLS1_3_MD_MAX_SIZE */

/* A device arena for single-shot calls: inputs are packed into one host
 * buffer, copied once, the job chain runs, the outputs come back. */
namespace {
struct Arena {
    uint8_t host[32768];
    size_t used = 0;
    size_t put(const void *p, size_t n)
    {
        size_t off = used;
        if (n && p) memcpy(host + off, p, n);
        else if (n) memset(host + off, 0, n);
        used = (used + n + 15) & ~(size_t) 15;
        return off;
    }
};
}

static pthread_mutex_t g_ks_mu = PTHREAD_MUTEX_INITIALIZER;
static hipStream_t g_ks_stream = nullptr;
static uint8_t *g_ks_dev = nullptr;          /* 32 KiB arena + job array */
static const size_t KS_DEV_BYTES = 32768 + 16 * sizeof(Job);

static int ks_init_locked(void)
{
    if (g_ks_dev) return 0;
    if (tlsrec_device_check() != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    if (hipStreamCreateWithFlags(&g_ks_stream, hipStreamNonBlocking) != hipSuccess) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    if (hipMalloc((void **) &g_ks_dev, KS_DEV_BYTES) != hipSuccess) {
        g_ks_dev = nullptr;
        return TLSREC_ERR_SSL_ALLOC_FAILED;
    }
    return 0;
}

/* tlsrec_internal.h: the arena for cookie.hip's batch of one */
int tlsrec_ks_arena_lock(uint8_t **dev, hipStream_t *stream)
{
    pthread_mutex_lock(&g_ks_mu);
    const int r = ks_init_locked();
    if (r != 0) {
        pthread_mutex_unlock(&g_ks_mu);
        return r;
    }
    *dev = g_ks_dev;
    *stream = g_ks_stream;
    return 0;
}

void tlsrec_ks_arena_unlock(void) { pthread_mutex_unlock(&g_ks_mu); }

/* Run `stages` dependent launches; stage s runs jobs [first[s], first[s+1]).
 * Job pointers are arena offsets (tagged with bit 63) rebased to the device. */
static const uint64_t OFF = 1ull << 62;
static inline const uint8_t *dev_off(size_t off) { return (const uint8_t *) (uintptr_t) (OFF | off); }

static int run_jobs(Arena &ar, Job *jobs, const int *first, int stages, const size_t *outs, void *const *host_out,
                    const size_t *out_len, int nouts)
{
    pthread_mutex_lock(&g_ks_mu);
    int r = ks_init_locked();
    if (r == 0) {
        const int njobs = first[stages];
        auto fix = [](const uint8_t *p) -> const uint8_t * {
            const uint64_t v = (uint64_t) (uintptr_t) p;
            return (v & OFF) ? g_ks_dev + (v & ~OFF) : p;
        };
        for (int i = 0; i < njobs; i++) {
            jobs[i].key = fix(jobs[i].key);
            jobs[i].msg = fix(jobs[i].msg);
            jobs[i].msg2 = fix(jobs[i].msg2);
            jobs[i].out = (uint8_t *) fix(jobs[i].out);
        }
        Job *djobs = (Job *) (g_ks_dev + 32768);
        hipError_t e = hipMemcpyAsync(g_ks_dev, ar.host, ar.used, hipMemcpyHostToDevice, g_ks_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(djobs, jobs, sizeof(Job) * njobs, hipMemcpyHostToDevice, g_ks_stream);
        for (int s = 0; s < stages && e == hipSuccess; s++) {
            const uint32_t n = (uint32_t) (first[s + 1] - first[s]);
            hipLaunchKernelGGL(kdf_job_kernel, dim3(1), dim3(64), 0, g_ks_stream, djobs + first[s], n);
            e = hipGetLastError();
        }
        for (int o = 0; o < nouts && e == hipSuccess; o++)
            e = hipMemcpyAsync(host_out[o], g_ks_dev + outs[o], out_len[o], hipMemcpyDeviceToHost, g_ks_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_ks_stream);
        /* wipe secrets from the device arena (ssl_tls13_keys.c zeroizes its temporaries) */
        hipMemsetAsync(g_ks_dev, 0, ar.used, g_ks_stream);
        hipStreamSynchronize(g_ks_stream);
        if (e != hipSuccess) r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    pthread_mutex_unlock(&g_ks_mu);
    memset(ar.host, 0, ar.used);
    return r;
}

static Job job(uint32_t op, int alg, size_t key, uint32_t key_len, size_t msg, uint32_t msg_len, size_t out,
               uint32_t out_len)
{
    Job j;
    memset(&j, 0, sizeof(j));
    j.op = op;
    j.alg = (uint32_t) alg;
    j.key = dev_off(key);
    j.key_len = key_len;
    j.msg = dev_off(msg);
    j.msg_len = msg_len;
    j.msg2 = dev_off(0);
    j.msg2_len = 0;
    j.out = (uint8_t *) dev_off(out);
    j.out_len = out_len;
    return j;
}

extern "C" int tlsrec_tls13_hkdf_expand_label(int hash_alg, const unsigned char *secret, size_t secret_len,
                                              const unsigned char *label, size_t label_len,
                                              const unsigned char *ctx, size_t ctx_len, unsigned char *buf,
                                              size_t buf_len)
{
    /* argument checks in the order of ssl_tls13_keys.c:152-171 */
    if (label_len > MAX_LABEL) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (ctx_len > MAX_CONTEXT) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (buf_len > MAX_EXPANSION) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (buf_len > 255 * alg_len(a)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;   /* HKDF-Expand limit (PSA: INVALID_ARGUMENT) */
    if (secret_len > 4096) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (buf_len == 0) return 0;
    Arena ar;
    uint8_t info[2 + 1 + 6 + 249 + 1 + 64];
    const size_t il = encode_label(buf_len, label, label_len, ctx, ctx_len, info);
    const size_t o_sec = ar.put(secret, secret_len), o_info = ar.put(info, il), o_out = ar.put(nullptr, buf_len);
    memset(info, 0, sizeof(info));
    if (ar.used > 32768) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Job j[1] = { job(OP_EXPAND, a, o_sec, (uint32_t) secret_len, o_info, (uint32_t) il, o_out, (uint32_t) buf_len) };
    const int first[2] = { 0, 1 };
    void *ho[1] = { buf };
    return run_jobs(ar, j, first, 1, &o_out, ho, &buf_len, 1);
}

/* Derive-Secret with the context hashed on the device: HASH(ctx) -> EXPAND
 * with info = HkdfLabel prefix || Hash(ctx). */
static int derive_secret_impl(int a, const unsigned char *secret, size_t secret_len, const unsigned char *label,
                              size_t label_len, const unsigned char *ctx, size_t ctx_len, int ctx_hashed,
                              unsigned char *dst, size_t dst_len)
{
    if (label_len > MAX_LABEL) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (ctx_hashed != TLSREC_TLS13_CONTEXT_UNHASHED && ctx_len > MAX_CONTEXT) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (dst_len > MAX_EXPANSION) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (dst_len > 255 * alg_len(a)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (secret_len > 4096 || (ctx_hashed == TLSREC_TLS13_CONTEXT_UNHASHED && ctx_len > 16384))
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (dst_len == 0) return 0;
    Arena ar;
    const size_t H = alg_len(a);
    uint8_t info[2 + 1 + 6 + 249 + 1 + 64];
    const size_t ctx_out = ctx_hashed == TLSREC_TLS13_CONTEXT_UNHASHED ? H : ctx_len;
    /* prefix up to and including the context-length byte */
    const size_t il = encode_label(dst_len, label, label_len, nullptr, ctx_out, info);
    const size_t o_sec = ar.put(secret, secret_len), o_info = ar.put(info, il);
    const size_t o_ctx = ar.put(ctx, ctx_len), o_hash = ar.put(nullptr, 64), o_out = ar.put(nullptr, dst_len);
    memset(info, 0, sizeof(info));
    if (ar.used > 32768) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Job j[2];
    int first[3];
    int stages;
    if (ctx_hashed == TLSREC_TLS13_CONTEXT_UNHASHED) {
        j[0] = job(OP_HASH, a, 0, 0, o_ctx, (uint32_t) ctx_len, o_hash, (uint32_t) H);
        j[1] = job(OP_EXPAND, a, o_sec, (uint32_t) secret_len, o_info, (uint32_t) il, o_out, (uint32_t) dst_len);
        j[1].msg2 = dev_off(o_hash);
        j[1].msg2_len = (uint32_t) H;
        first[0] = 0; first[1] = 1; first[2] = 2;
        stages = 2;
    } else {
        j[0] = job(OP_EXPAND, a, o_sec, (uint32_t) secret_len, o_info, (uint32_t) il, o_out, (uint32_t) dst_len);
        j[0].msg2 = dev_off(o_ctx);
        j[0].msg2_len = (uint32_t) ctx_len;
        first[0] = 0; first[1] = 1;
        stages = 1;
    }
    void *ho[1] = { dst };
    return run_jobs(ar, j, first, stages, &o_out, ho, &dst_len, 1);
}

extern "C" int tlsrec_tls13_derive_secret(int hash_alg, const unsigned char *secret, size_t secret_len,
                                          const unsigned char *label, size_t label_len, const unsigned char *ctx,
                                          size_t ctx_len, int ctx_hashed, unsigned char *dstbuf, size_t dstbuf_len)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return derive_secret_impl(a, secret, secret_len, label, label_len, ctx, ctx_len, ctx_hashed, dstbuf, dstbuf_len);
}

extern "C" int tlsrec_tls13_evolve_secret(int hash_alg, const unsigned char *secret_old, const unsigned char *input,
                                          size_t input_len, unsigned char *secret_new)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t H = alg_len(a);
    if (input_len > 16384) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Arena ar;
    uint8_t info[32];
    const size_t il = encode_label(H, (const unsigned char *) "derived", 7, nullptr, H, info);
    const size_t o_old = ar.put(secret_old, secret_old ? H : 0), o_info = ar.put(info, il);
    const size_t o_empty = ar.put(nullptr, 0), o_hash = ar.put(nullptr, 64), o_tmp = ar.put(nullptr, 64);
    const bool have_in = input != NULL && input_len != 0;
    const size_t o_in = ar.put(have_in ? input : nullptr, have_in ? input_len : H);   /* zeros when absent */
    const size_t o_out = ar.put(nullptr, 64);
    Job j[3];
    int first[4];
    int stages = 0, k = 0;
    first[0] = 0;
    if (secret_old) {
        /* Derive-Secret(secret_old, "derived", "") -> tmp (ssl_tls13_keys.c:358-369) */
        j[k++] = job(OP_HASH, a, 0, 0, o_empty, 0, o_hash, (uint32_t) H);
        first[++stages] = k;
        j[k] = job(OP_EXPAND, a, o_old, (uint32_t) H, o_info, (uint32_t) il, o_tmp, (uint32_t) H);
        j[k].msg2 = dev_off(o_hash);
        j[k++].msg2_len = (uint32_t) H;
        first[++stages] = k;
    }
    /* HKDF-Extract(salt = tmp (zeros for the first stage), IKM) */
    j[k++] = job(OP_HMAC, a, o_tmp, (uint32_t) H, o_in, (uint32_t) (have_in ? input_len : H), o_out, (uint32_t) H);
    first[++stages] = k;
    void *ho[1] = { secret_new };
    return run_jobs(ar, j, first, stages, &o_out, ho, &H, 1);
}

extern "C" int tlsrec_tls13_make_traffic_keys(int hash_alg, const unsigned char *client_secret,
                                              const unsigned char *server_secret, size_t secret_len, size_t key_len,
                                              size_t iv_len, tlsrec_key_set *keys)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!keys || key_len > sizeof(keys->client_write_key) || iv_len > sizeof(keys->client_write_iv))
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (secret_len > 4096) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Arena ar;
    uint8_t ik[32], iv[32];
    const size_t lk = encode_label(key_len, (const unsigned char *) "key", 3, nullptr, 0, ik);
    const size_t lv = encode_label(iv_len, (const unsigned char *) "iv", 2, nullptr, 0, iv);
    const size_t o_c = ar.put(client_secret, secret_len), o_s = ar.put(server_secret, secret_len);
    const size_t o_ik = ar.put(ik, lk), o_iv = ar.put(iv, lv);
    const size_t o_ck = ar.put(nullptr, 32), o_ci = ar.put(nullptr, 16), o_sk = ar.put(nullptr, 32),
                 o_si = ar.put(nullptr, 16);
    Job j[4] = { job(OP_EXPAND, a, o_c, (uint32_t) secret_len, o_ik, (uint32_t) lk, o_ck, (uint32_t) key_len),
                 job(OP_EXPAND, a, o_c, (uint32_t) secret_len, o_iv, (uint32_t) lv, o_ci, (uint32_t) iv_len),
                 job(OP_EXPAND, a, o_s, (uint32_t) secret_len, o_ik, (uint32_t) lk, o_sk, (uint32_t) key_len),
                 job(OP_EXPAND, a, o_s, (uint32_t) secret_len, o_iv, (uint32_t) lv, o_si, (uint32_t) iv_len) };
    const int first[2] = { 0, 4 };
    const size_t outs[4] = { o_ck, o_ci, o_sk, o_si };
    void *ho[4] = { keys->client_write_key, keys->client_write_iv, keys->server_write_key, keys->server_write_iv };
    const size_t ol[4] = { key_len, iv_len, key_len, iv_len };
    int r = run_jobs(ar, j, first, 1, outs, ho, ol, 4);
    if (r == 0) {
        keys->key_len = key_len;
        keys->iv_len = iv_len;
    }
    return r;
}

extern "C" int tlsrec_tls13_exporter(int hash_alg, const unsigned char *secret, size_t secret_len,
                                     const unsigned char *label, size_t label_len,
                                     const unsigned char *context_value, size_t context_len, unsigned char *out,
                                     size_t out_len)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t H = alg_len(a);
    uint8_t s[64];
    /* ssl_tls13_keys.c:1836-1852: two Derive-Secret steps, unhashed contexts */
    int r = derive_secret_impl(a, secret, secret_len, label, label_len, nullptr, 0, TLSREC_TLS13_CONTEXT_UNHASHED,
                               s, H);
    if (r == 0)
        r = derive_secret_impl(a, s, H, (const unsigned char *) "exporter", 8, context_value, context_len,
                               TLSREC_TLS13_CONTEXT_UNHASHED, out, out_len);
    volatile uint8_t *v = s;
    for (size_t i = 0; i < sizeof(s); i++) v[i] = 0;
    return r;
}

extern "C" int tlsrec_tls13_update_traffic_secret(int hash_alg, const unsigned char *secret, unsigned char *next)
{
    const int a = alg_index(hash_alg);
    if (a < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t H = alg_len(a);
    return tlsrec_tls13_hkdf_expand_label(hash_alg, secret, H, (const unsigned char *) "traffic upd", 11, nullptr, 0,
                                          next, H);
}


/* The derive kernel alone: key material of `count` slots into the staging
 * area, nothing committed (tools/bench_keysched.py times it apart from the
 * key setup; tlsrec_tls13_keytab_derive is this + the commit). */
extern "C" int tlsrec__tls13_stage_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                        tlsrec_tls13_secret *secrets, int key_update, void *stream)
{
    if (!kt || (!secrets && count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!keytab_range_ok(kt, first, count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    uint32_t key_len, alg;
    /* TLS 1.3 suites fix the hash with the AEAD (RFC 8446 B.4):
     * TLS_AES_256_GCM_SHA384, every other suite SHA-256 */
    key_len = tlsrec_cipher_keylen(cipher);
    if (key_len == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    alg = cipher == TLSREC_CIPHER_AES_256_GCM ? H_SHA384 : H_SHA256;
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    uint8_t infos[96];
    const uint32_t H = (uint32_t) alg_len((int) alg);
    const size_t lu = encode_label(H, (const unsigned char *) "traffic upd", 11, nullptr, 0, infos);
    const size_t lk = encode_label(key_len, (const unsigned char *) "key", 3, nullptr, 0, infos + lu);
    const size_t lv = encode_label(12, (const unsigned char *) "iv", 2, nullptr, 0, infos + lu + lk);
    DeriveArgs a;
    a.secrets = secrets;
    a.out = tlsrec__keytab_stage(kt) + first;
    memcpy(a.infos, infos, sizeof(a.infos));
    a.len_upd = (uint32_t) lu;
    a.len_key = (uint32_t) lk;
    a.len_iv = (uint32_t) lv;
    a.count = count;
    a.alg = alg;
    a.cipher = (uint32_t) cipher;
    a.key_len = key_len;
    a.update = key_update ? 1u : 0u;
    hipLaunchKernelGGL(tls13_derive_kernel, dim3((count + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_tls13_keytab_derive(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                          tlsrec_tls13_secret *secrets, int key_update, void *stream)
{
    int r = tlsrec__tls13_stage_keys(kt, first, count, cipher, secrets, key_update, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, count, cipher, (hipStream_t) stream);
    return r;
}

/* ---- the rest of the ladder, single-shot (ssl_tls13_keys.c:421-650, :697, :832) ----
 * Compositions of the calls above on the kdf_job_kernel path. */
static int ladder_alg(int hash_alg, int *a)
{
    /* the reference's "!PSA_ALG_IS_HASH(hash_alg)" assertion, then the hashes this library has */
    if (((uint32_t) hash_alg & 0x7f000000u) != 0x02000000u) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    *a = alg_index(hash_alg);
    return *a < 0 ? TLSREC_ERR_SSL_BAD_INPUT_DATA : 0;
}

static int ladder_derive(int a, const unsigned char *secret, const char *label, const unsigned char *transcript,
                         size_t transcript_len, unsigned char *dst)
{
    return derive_secret_impl(a, secret, alg_len(a), (const unsigned char *) label, strlen(label), transcript,
                              transcript_len, TLSREC_TLS13_CONTEXT_HASHED, dst, alg_len(a));
}

extern "C" int tlsrec_tls13_derive_early_secrets(int hash_alg, const unsigned char *early_secret,
                                                 const unsigned char *transcript, size_t transcript_len,
                                                 tlsrec_tls13_early_secrets *derived)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!early_secret || !derived || (!transcript && transcript_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    r = ladder_derive(a, early_secret, "c e traffic", transcript, transcript_len, derived->client_early_traffic_secret);
    if (r == 0)
        r = ladder_derive(a, early_secret, "e exp master", transcript, transcript_len,
                          derived->early_exporter_master_secret);
    return r;
}

extern "C" int tlsrec_tls13_derive_handshake_secrets(int hash_alg, const unsigned char *handshake_secret,
                                                     const unsigned char *transcript, size_t transcript_len,
                                                     tlsrec_tls13_handshake_secrets *derived)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!handshake_secret || !derived || (!transcript && transcript_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    r = ladder_derive(a, handshake_secret, "c hs traffic", transcript, transcript_len,
                      derived->client_handshake_traffic_secret);
    if (r == 0)
        r = ladder_derive(a, handshake_secret, "s hs traffic", transcript, transcript_len,
                          derived->server_handshake_traffic_secret);
    return r;
}

extern "C" int tlsrec_tls13_derive_application_secrets(int hash_alg, const unsigned char *application_secret,
                                                       const unsigned char *transcript, size_t transcript_len,
                                                       tlsrec_tls13_application_secrets *derived)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!application_secret || !derived || (!transcript && transcript_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    r = ladder_derive(a, application_secret, "c ap traffic", transcript, transcript_len,
                      derived->client_application_traffic_secret_N);
    if (r == 0)
        r = ladder_derive(a, application_secret, "s ap traffic", transcript, transcript_len,
                          derived->server_application_traffic_secret_N);
    if (r == 0)
        r = ladder_derive(a, application_secret, "exp master", transcript, transcript_len,
                          derived->exporter_master_secret);
    return r;
}

extern "C" int tlsrec_tls13_derive_resumption_master_secret(int hash_alg, const unsigned char *application_secret,
                                                            const unsigned char *transcript, size_t transcript_len,
                                                            tlsrec_tls13_application_secrets *derived)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!application_secret || !derived || (!transcript && transcript_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return ladder_derive(a, application_secret, "res master", transcript, transcript_len,
                         derived->resumption_master_secret);
}

/* ssl_tls13_calc_finished_core: EXPAND "finished" -> HMAC over the transcript hash, one job chain */
static int calc_finished_impl(int a, const unsigned char *base, const unsigned char *transcript, unsigned char *dst)
{
    const size_t H = alg_len(a);
    Arena ar;
    uint8_t info[32];
    const size_t il = encode_label(H, (const unsigned char *) "finished", 8, nullptr, 0, info);
    const size_t o_base = ar.put(base, H), o_info = ar.put(info, il), o_tr = ar.put(transcript, H);
    const size_t o_key = ar.put(nullptr, 64), o_out = ar.put(nullptr, 64);
    Job j[2] = { job(OP_EXPAND, a, o_base, (uint32_t) H, o_info, (uint32_t) il, o_key, (uint32_t) H),
                 job(OP_HMAC, a, o_key, (uint32_t) H, o_tr, (uint32_t) H, o_out, (uint32_t) H) };
    const int first[3] = { 0, 1, 2 };
    void *ho[1] = { dst };
    return run_jobs(ar, j, first, 2, &o_out, ho, &H, 1);
}

extern "C" int tlsrec_tls13_calc_finished(int hash_alg, const unsigned char *base_secret,
                                          const unsigned char *transcript, unsigned char *out, size_t *out_len)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if (!base_secret || !transcript || !out || !out_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    r = calc_finished_impl(a, base_secret, transcript, out);
    if (r == 0) *out_len = alg_len(a);
    return r;
}

extern "C" int tlsrec_tls13_create_psk_binder(int hash_alg, const unsigned char *psk, size_t psk_len, int psk_type,
                                              const unsigned char *transcript, unsigned char *result)
{
    int a, r = ladder_alg(hash_alg, &a);
    if (r) return r;
    if ((!psk && psk_len) || !transcript || !result) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    uint8_t early[64], binder_key[64];
    r = tlsrec_tls13_evolve_secret(hash_alg, nullptr, psk, psk_len, early);
    /* ssl_tls13_keys.c:879-895: "res binder" for a resumption PSK, "ext binder" for any other type */
    const char *lbl = psk_type == TLSREC_TLS13_PSK_RESUMPTION ? "res binder" : "ext binder";
    if (r == 0)
        r = derive_secret_impl(a, early, alg_len(a), (const unsigned char *) lbl, 10, nullptr, 0,
                               TLSREC_TLS13_CONTEXT_UNHASHED, binder_key, alg_len(a));
    if (r == 0) r = calc_finished_impl(a, binder_key, transcript, result);
    volatile uint8_t *v = early, *u = binder_key;
    for (size_t i = 0; i < 64; i++) { v[i] = 0; u[i] = 0; }
    return r;
}

/* ======================================================================
 * TLS 1.2 / DTLS 1.2 (library/ssl_tls.c), single-shot
 *
 *   reference                                        here
 *   mbedtls_ssl_tls_prf               :465           tlsrec_tls_prf
 *   tls_prf_generic                   :6099          OP_PRF (tls_prf() above)
 *   ssl_compute_master                :6251-6451     tlsrec_tls12_compute_master (non-PSK branch)
 *   tls_prf(.., "key expansion", ..)  :7750          tlsrec_tls12_make_keys, _make_keys_cbc
 *                                                    (the key-block split: tls12_batch.hip)
 *   ssl_calc_finished_tls_generic     :7209-7261     tlsrec_tls12_calc_finished
 *   mbedtls_ssl_tls12_export_keying_material :8886   tlsrec_tls12_export_keying_material
 * ==================================================================== */
/* PRF with seed = label || r1 || r2 through the arena (a = H_SHA256 / H_SHA384) */
static int prf_run(int a, const unsigned char *secret, size_t slen, const char *label, size_t llen,
                   const unsigned char *r1, size_t r1len, const unsigned char *r2, size_t r2len,
                   unsigned char *dst, size_t dlen)
{
    if ((slen && !secret) || (llen && !label) || (r1len && !r1) || (r2len && !r2) || !dst)
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* the arena holds the secret, the label, the random bytes and the output, each rounded to 16 bytes */
    const size_t lim = 32768;
    if (slen > lim || llen > lim || r1len > lim || r2len > lim || dlen > lim) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t rlen = r1len + r2len;
    if (((slen + 15) & ~(size_t) 15) + ((llen + 15) & ~(size_t) 15) + ((rlen + 15) & ~(size_t) 15) +
        ((dlen + 15) & ~(size_t) 15) > lim)
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    Arena ar;
    const size_t o_sec = ar.put(secret, slen), o_lab = ar.put(label, llen);
    const size_t o_rnd = ar.used;
    if (r1len) memcpy(ar.host + o_rnd, r1, r1len);
    if (r2len) memcpy(ar.host + o_rnd + r1len, r2, r2len);
    ar.used = (ar.used + rlen + 15) & ~(size_t) 15;
    const size_t o_out = ar.put(nullptr, dlen);
    Job j[1] = { job(OP_PRF, a, o_sec, (uint32_t) slen, o_lab, (uint32_t) llen, o_out, (uint32_t) dlen) };
    j[0].msg2 = dev_off(o_rnd);
    j[0].msg2_len = (uint32_t) rlen;
    const int first[2] = { 0, 1 };
    void *ho[1] = { dst };
    return run_jobs(ar, j, first, 1, &o_out, ho, &dlen, 1);
}

extern "C" int tlsrec_tls_prf(int prf, const unsigned char *secret, size_t slen, const char *label,
                              const unsigned char *random, size_t rlen, unsigned char *dstbuf, size_t dlen)
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;      /* ssl_tls.c:489-490 */
    if (dlen == 0) return 0;
    if (!label) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return prf_run(a, secret, slen, label, strlen(label), random, rlen, nullptr, 0, dstbuf, dlen);
}

extern "C" int tlsrec_tls12_compute_master(int prf, const unsigned char *premaster, size_t pmslen,
                                           const unsigned char *seed, size_t seed_len, int extended_ms,
                                           unsigned char master[48])
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    /* ssl_tls.c:6269, :6295 */
    const char *lbl = extended_ms ? "extended master secret" : "master secret";
    return prf_run(a, premaster, pmslen, lbl, strlen(lbl), seed, seed_len, nullptr, 0, master, 48);
}

extern "C" int tlsrec_tls12_make_keys(int prf, int cipher, const unsigned char master[48],
                                      const unsigned char randbytes[64], tlsrec_key_set *keys)
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    const size_t kl = tlsrec_cipher_keylen(cipher);
    if (kl == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (!master || !randbytes || !keys) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* the reference expands 256 bytes (ssl_tls.c:7750) and uses this prefix of them */
    unsigned char keyblk[96];
    const size_t need = 2 * kl + 2 * tls12_fixed_ivlen(cipher);
    int r = prf_run(a, master, 48, "key expansion", 13, randbytes, 64, nullptr, 0, keyblk, need);
    if (r == 0) r = tlsrec_tls12_split_key_block(cipher, keyblk, need, keys);
    wipe(keyblk, sizeof(keyblk));
    return r;
}

extern "C" int tlsrec_tls12_make_keys_cbc(int prf, int cipher, int mac, const unsigned char master[48],
                                          const unsigned char randbytes[64], tlsrec_cbc_key_set *out)
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    const size_t kl = cbc_split_keylen(cipher), ml = cbc_split_maclen(mac);
    if (!cbc_split_pair_ok(cipher, mac)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (!master || !randbytes || !out) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    unsigned char keyblk[160];
    const size_t need = 2 * ml + 2 * kl;
    int r = prf_run(a, master, 48, "key expansion", 13, randbytes, 64, nullptr, 0, keyblk, need);
    if (r == 0) r = tlsrec_tls12_split_key_block_cbc(cipher, mac, keyblk, need, out);
    wipe(keyblk, sizeof(keyblk));
    return r;
}

extern "C" int tlsrec_tls12_export_keying_material(int prf, const unsigned char master[48],
                                                   const unsigned char randbytes[64], const char *label,
                                                   size_t label_len, const unsigned char *context,
                                                   size_t context_len, int use_context, unsigned char *out,
                                                   size_t out_len)
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (use_context && context_len > 65535) return TLSREC_ERR_SSL_BAD_INPUT_DATA;     /* ssl_tls.c:8905 */
    if (out_len == 0) return 0;
    if (!master || !randbytes || (use_context && context_len && !context)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* client_random || server_random [|| uint16 context_len || context], ssl_tls.c:8920-8929 */
    unsigned char head[66];
    memcpy(head, randbytes + 32, 32);
    memcpy(head + 32, randbytes, 32);
    head[64] = (unsigned char) (context_len >> 8);
    head[65] = (unsigned char) context_len;
    return prf_run(a, master, 48, label, label_len, head, use_context ? 66 : 64, context,
                   use_context ? context_len : 0, out, out_len);
}

extern "C" int tlsrec_tls12_calc_finished(int prf, const unsigned char master[48], const unsigned char *transcript_hash,
                                          int from, unsigned char out[12])
{
    const int a = prf_index(prf);
    if (a < 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (from != TLSREC_IS_CLIENT && from != TLSREC_IS_SERVER) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!master || !transcript_hash || !out) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* ssl_tls.c:7217-7219, :7252 */
    const char *lbl = from == TLSREC_IS_CLIENT ? "client finished" : "server finished";
    return prf_run(a, master, 48, lbl, 15, transcript_hash, alg_len(a), nullptr, 0, out, 12);
}

