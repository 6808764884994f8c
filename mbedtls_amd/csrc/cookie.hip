/*
 * cookie.hip -- the DTLS cookie exchange on the GPU, one client per lane, on
 * the word-wise HMAC-SHA256 blocks of tlsrec_kdf.h:
 *
 *   reference                                             here
 *   mbedtls_ssl_cookie_setup / _set_timeout / _free
 *                                (library/ssl_cookie.c)   tlsrec_cookie_setup, _set_timeout, _free
 *   mbedtls_ssl_cookie_write / _check                     tlsrec_cookie_write, _check,
 *                                                         tlsrec_cookie_batch_write, _batch_check
 *   mbedtls_ssl_check_dtls_clihlo_cookie
 *                     (library/ssl_msg.c:3322-3454)       tlsrec_dtls_check_clihlo_cookies
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>
#include <time.h>

#include "tlsrec.h"
#include "tlsrec_internal.h"
#include "tlsrec_kdf.h"

namespace tlsks {

/* ======================================================================
 * DTLS cookies (library/ssl_cookie.c, ssl_msg.c:3322-3454)
 * ====================================================================== */
/* mbedtls_ssl_cookie_write / _check and mbedtls_ssl_check_dtls_clihlo_cookie,
 * one client per lane, all under the one key whose two HMAC midstates the
 * context holds (uniform loads: scalar registers, read once per wave).
 *     cookie = BE32(t) || HMAC-SHA256(key, BE32(t) || id)[0..28)
 * The inner message is 4 + id_len bytes: one block up to an id of 51 bytes
 * (an IPv4 or IPv6 address with its port), built with constant word indices;
 * a longer id takes further blocks in a loop whose trip count differs between
 * the lanes of a wave.  Compressions per item: write and check 2 (+1 per
 * further block), a ClientHello 2 when its cookie passes or cannot be one
 * (length != 32), 4 when a 32-byte cookie fails.  The kernel has one MAC site:
 * in a wave of ClientHellos the lanes that check and the lanes that only
 * write run it together, and only a failed 32-byte cookie costs a second trip. */
enum { CK_WRITE = 0, CK_CHECK = 1, CK_HELLO = 2 };

struct CookieArgs {
    const uint32_t *mid;          /* ip[8], op[8] */
    const void *items;            /* tlsrec_cookie_item / tlsrec_clihlo */
    const uint8_t *arena;         /* check: the cookies; hello: the datagrams */
    const uint8_t *id_arena;
    uint8_t *out;                 /* write: the cookies; hello: the HelloVerifyRequests */
    int32_t *status;              /* int32 per item; hello: tlsrec_clihlo_res */
    uint64_t now;
    uint32_t timeout, n;
};

/* fail closed: what the kernel does not reach reads INTERNAL_ERROR (words = int32s per result) */
__global__ void __launch_bounds__(64) cookie_prefill_kernel(int32_t *status, uint32_t n, uint32_t words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    status[(size_t) i * words] = TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (words == 2) status[(size_t) i * 2 + 1] = 0;
}

/* the key's midstates, once per context; the staged key is zeroed behind them */
__global__ void __launch_bounds__(64) cookie_setup_kernel(uint32_t *mid, uint8_t *key)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t k[8], ip[8], op[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = load_be32(key + 4 * j, false);
    hmac_mid<L256>(k, ip, op);
#pragma unroll
    for (int j = 0; j < 8; j++) { mid[j] = ip[j]; mid[8 + j] = op[j]; }
    for (int j = 0; j < 32; j++) key[j] = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { k[j] = 0; ip[j] = 0; op[j] = 0; }
}

/* big-endian word of the padded id at byte p: id bytes below id_len (no byte
 * at or past it is read), 0x80 at id_len, zero after */
__device__ __forceinline__ uint32_t cookie_id_word(const uint8_t *id, int p, int id_len)
{
    const int rem = id_len - p;
    uint32_t v = 0;
    if (rem >= 4) {
        v = load_be32(id + p, false);
    } else if (rem >= 0) {
        if (rem > 0) v |= (uint32_t) id[p] << 24;
        if (rem > 1) v |= (uint32_t) id[p + 1] << 16;
        if (rem > 2) v |= (uint32_t) id[p + 2] << 8;
        v |= 0x80u << (24 - 8 * rem);
    }
    return v;
}

/* HMAC-SHA256(key, BE32(t) || id) from the midstates; mac[0..7) is the cookie's MAC */
__device__ __forceinline__ void cookie_mac(const uint32_t (&ip)[8], const uint32_t (&op)[8], uint32_t t,
                                           const uint8_t *id, uint32_t id_len, uint32_t (&mac)[8])
{
    uint32_t st[8], w[16];
    const uint32_t n = 4 + id_len, nblk = (n + 9 + 63) >> 6;
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = ip[j];
    w[0] = t;
#pragma unroll
    for (int c = 1; c < 16; c++) w[c] = cookie_id_word(id, 4 * c - 4, (int) id_len);
    if (nblk == 1) w[15] = (64 + n) * 8;
    sha_compress<S256>(st, w);
#pragma unroll 1
    for (uint32_t b = 1; b < nblk; b++) {
#pragma unroll
        for (int c = 0; c < 16; c++) w[c] = cookie_id_word(id, (int) (64 * b) + 4 * c - 4, (int) id_len);
        if (b == nblk - 1) w[15] = (64 + n) * 8;
        sha_compress<S256>(st, w);
    }
    hmac_outer<L256>(op, st, mac);
}

/* N big-endian words to any address: 4-byte stores, or bytes */
template <int N> __device__ __forceinline__ void cookie_store(uint8_t *p, const uint32_t (&v)[N])
{
    if (((uintptr_t) p & 3) == 0) {
#pragma unroll
        for (int c = 0; c < N; c++) reinterpret_cast<uint32_t *>(p)[c] = __builtin_bswap32(v[c]);
    } else {
#pragma unroll
        for (int c = 0; c < N; c++) {
            p[4 * c] = (uint8_t) (v[c] >> 24); p[4 * c + 1] = (uint8_t) (v[c] >> 16);
            p[4 * c + 2] = (uint8_t) (v[c] >> 8); p[4 * c + 3] = (uint8_t) v[c];
        }
    }
}

/* a ClientHello whose cookie did not pass: the buffer checks of ssl_msg.c:3424 and of f_cookie_write
 * (:3436-3440; it also refuses an id it cannot take); write = a HelloVerifyRequest follows */
__device__ __forceinline__ void cookie_hvr_room(uint32_t out_cap, uint32_t id_len, int32_t &st, bool &write)
{
    st = out_cap < 28 ? TLSREC_ERR_SSL_BUFFER_TOO_SMALL : TLSREC_ERR_SSL_INTERNAL_ERROR;
    write = out_cap >= TLSREC_DTLS_HVR_LEN && id_len <= 255;
}

template <int MODE> __global__ void __launch_bounds__(64) cookie_kernel(CookieArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    uint32_t ip[8], op[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = a.mid[j]; op[j] = a.mid[8 + j]; }
    const uint32_t now32 = (uint32_t) a.now;                     /* MBEDTLS_PUT_UINT32_BE(t), ssl_cookie.c:140 */

    const uint8_t *id, *in = nullptr;
    uint8_t *out = nullptr;
    uint32_t id_len, out_cap = 0;
    uint32_t C[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };          /* the received cookie */
    int32_t st = 0;
    bool check = false, write = false;
    if constexpr (MODE == CK_HELLO) {
        const tlsrec_clihlo h = static_cast<const tlsrec_clihlo *>(a.items)[i];
        in = a.arena + h.off;
        id = a.id_arena + h.id_off;
        id_len = h.id_len;
        out = a.out + h.out_off;
        out_cap = h.out_cap;
        const uint32_t len = h.len;
        /* ssl_msg.c:3360-3393; every byte read lies below len */
        bool bad = len < 61;
        uint32_t ck_at = 0, ck_len = 0;
        if (!bad) {
            const uint32_t epoch = ((uint32_t) in[3] << 8) | in[4];
            const uint32_t frag = ((uint32_t) in[19] << 16) | ((uint32_t) in[20] << 8) | in[21];
            const uint32_t sid_len = in[59];
            bad = in[0] != 22 || epoch != 0 || frag != 0 || 61 + sid_len > len;
            if (!bad) {
                ck_len = in[60 + sid_len];
                ck_at = 61 + sid_len;
                bad = ck_at + ck_len > len;
            }
        }
        if (bad) {
            st = TLSREC_ERR_SSL_DECODE_ERROR;
        } else if (ck_len == TLSREC_COOKIE_LEN && id_len <= 255) {
            const uint8_t *ck = in + ck_at;
            const bool al4 = ((uintptr_t) ck & 3) == 0;
#pragma unroll
            for (int c = 0; c < 8; c++) C[c] = load_be32(ck + 4 * c, al4);
            check = true;
        } else {
            write = true;        /* f_cookie_check != 0: the HelloVerifyRequest path */
        }
    } else {
        const tlsrec_cookie_item it = static_cast<const tlsrec_cookie_item *>(a.items)[i];
        id = a.id_arena + it.id_off;
        id_len = it.id_len;
        if (id_len > 255) {
            st = TLSREC_ERR_SSL_BAD_INPUT_DATA;
        } else if (MODE == CK_WRITE) {
            out = a.out + it.cookie_off;
            if (it.cookie_len < TLSREC_COOKIE_LEN) st = TLSREC_ERR_SSL_BUFFER_TOO_SMALL;     /* ssl_cookie.c:132 */
            else write = true;
        } else if (it.cookie_len != TLSREC_COOKIE_LEN) {
            st = -1;                                                                         /* ssl_cookie.c:198-200 */
        } else {
            const uint8_t *ck = a.arena + it.cookie_off;
            const bool al4 = ((uintptr_t) ck & 3) == 0;
#pragma unroll
            for (int c = 0; c < 8; c++) C[c] = load_be32(ck + 4 * c, al4);
            check = true;
        }
    }

    /* One MAC site, at most two passes.  Pass 0: the lanes with a cookie to check hash under its time
     * stamp, the lanes that only write (no cookie of 32 bytes came) under `now`, side by side.  Pass 1
     * (ClientHellos only): the lanes whose cookie failed hash again under `now` for the new cookie. */
    uint32_t olen = 0;
    uint32_t mac[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    if (MODE == CK_HELLO && write) cookie_hvr_room(out_cap, id_len, st, write);
#pragma unroll 1
    for (int pass = 0; pass < (MODE == CK_HELLO ? 2 : 1); pass++) {
        const bool chk = MODE != CK_WRITE && pass == 0 && check;
        if (!chk && !(MODE != CK_CHECK && write)) continue;
        cookie_mac(ip, op, chk ? C[0] : now32, id, id_len, mac);
        if (chk) {
            /* mbedtls_ct_memcmp over 28 bytes: the OR of the XOR of the seven words, no early exit; the
             * statuses are selected, not branched on (ssl_cookie.c:222-242) */
            uint32_t d = 0;
#pragma unroll
            for (int c = 0; c < 7; c++) d |= mac[c] ^ C[1 + c];
            const uint64_t age = a.now - (uint64_t) C[0];
            const int32_t late = (a.timeout != 0 && age > (uint64_t) a.timeout) ? -1 : 0;
            st = d != 0 ? TLSREC_ERR_SSL_INVALID_MAC : late;
            if (MODE == CK_HELLO && st != 0) cookie_hvr_room(out_cap, id_len, st, write);
        } else if (MODE == CK_WRITE) {
            const uint32_t o[8] = { now32, mac[0], mac[1], mac[2], mac[3], mac[4], mac[5], mac[6] };
            cookie_store<8>(out, o);
            write = false;
        } else {
            /* ssl_msg.c:3429-3451 with olen = 60: bytes 0-10 and 17-21 of the input, length 47, type 3,
             * length and fragment_length 35, FE FF, cookie length 32, the cookie */
            uint32_t b[25];
#pragma unroll
            for (int k = 0; k < 25; k++) b[k] = (k < 11 || (k >= 17 && k < 22)) ? in[k] : 0u;
            const uint32_t o[15] = {
                (b[0] << 24) | (b[1] << 16) | (b[2] << 8) | b[3],
                (b[4] << 24) | (b[5] << 16) | (b[6] << 8) | b[7],
                (b[8] << 24) | (b[9] << 16) | (b[10] << 8),
                ((TLSREC_DTLS_HVR_LEN - 13u) << 24) | (3u << 16),
                ((TLSREC_DTLS_HVR_LEN - 25u) << 24) | (b[17] << 16) | (b[18] << 8) | b[19],
                (b[20] << 24) | (b[21] << 16),
                ((TLSREC_DTLS_HVR_LEN - 25u) << 24) | 0x00feff00u | TLSREC_COOKIE_LEN,
                now32, mac[0], mac[1], mac[2], mac[3], mac[4], mac[5], mac[6] };
            cookie_store<15>(out, o);
            st = TLSREC_ERR_SSL_HELLO_VERIFY_REQUIRED;
            olen = TLSREC_DTLS_HVR_LEN;
            write = false;
        }
    }
    if (MODE == CK_HELLO) {
        a.status[2 * (size_t) i] = st;
        a.status[2 * (size_t) i + 1] = (int32_t) olen;
    } else {
        a.status[i] = st;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; mac[j] = 0; }
}

} /* namespace tlsks */

using namespace tlsks;

/* ---- DTLS cookies (library/ssl_cookie.c; ssl_msg.c:3322-3454) ---- */
struct tlsrec_cookie_ctx {
    uint32_t *mid;          /* device: ip[8], op[8], then the 32 bytes the key is staged in */
    uint32_t timeout;       /* ctx->timeout */
};

extern "C" int tlsrec_cookie_setup(tlsrec_cookie_ctx **ctx, const unsigned char key[32], uint32_t timeout)
{
    if (!ctx) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    *ctx = nullptr;
    if (tlsrec_device_check() != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    unsigned char k[32];
    if (key) {
        memcpy(k, key, 32);
    } else {
        /* psa_generate_key (ssl_cookie.c:105) */
        for (size_t got = 0; got < sizeof(k);) {
            const ssize_t r = getrandom(k + got, sizeof(k) - got, 0);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) {
                wipe(k, sizeof(k));
                return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
            }
            got += (size_t) r;
        }
    }
    tlsrec_cookie_ctx *c = (tlsrec_cookie_ctx *) calloc(1, sizeof(*c));
    int r = c ? 0 : TLSREC_ERR_SSL_ALLOC_FAILED;
    if (r == 0 && hipMalloc((void **) &c->mid, 64 + 32) != hipSuccess) {
        c->mid = nullptr;
        r = TLSREC_ERR_SSL_ALLOC_FAILED;
    }
    if (r == 0) {
        uint8_t *dkey = (uint8_t *) (c->mid + 16);
        hipError_t e = hipMemcpy(dkey, k, 32, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(cookie_setup_kernel, dim3(1), dim3(64), 0, (hipStream_t) nullptr, c->mid, dkey);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    wipe(k, sizeof(k));
    if (r != 0) {
        tlsrec_cookie_free(c);
        return r;
    }
    c->timeout = timeout;
    *ctx = c;
    return 0;
}

extern "C" void tlsrec_cookie_set_timeout(tlsrec_cookie_ctx *ctx, uint32_t delay)
{
    if (ctx) ctx->timeout = delay;
}

extern "C" void tlsrec_cookie_free(tlsrec_cookie_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->mid) {
        hipMemset(ctx->mid, 0, 64 + 32);
        hipDeviceSynchronize();
        hipFree(ctx->mid);
    }
    wipe(ctx, sizeof(*ctx));
    free(ctx);
}

static int cookie_launch(int mode, const tlsrec_cookie_ctx *ctx, uint64_t now, const void *items, uint32_t n,
                         const uint8_t *arena, const uint8_t *id_arena, uint8_t *out, int32_t *status, bool prefill,
                         hipStream_t st)
{
    CookieArgs a;
    a.mid = ctx->mid;
    a.items = items;
    a.arena = arena;
    a.id_arena = id_arena;
    a.out = out;
    a.status = status;
    a.now = now;
    a.timeout = ctx->timeout;
    a.n = n;
    const dim3 grid((n + 63) / 64), block(64);
    if (prefill)
        hipLaunchKernelGGL(cookie_prefill_kernel, grid, block, 0, st, status, n, mode == CK_HELLO ? 2u : 1u);
    if (mode == CK_WRITE) hipLaunchKernelGGL(cookie_kernel<CK_WRITE>, grid, block, 0, st, a);
    else if (mode == CK_CHECK) hipLaunchKernelGGL(cookie_kernel<CK_CHECK>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(cookie_kernel<CK_HELLO>, grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

extern "C" int tlsrec_cookie_batch_write(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_cookie_item *items,
                                         uint32_t n, const uint8_t *id_arena, uint8_t *cookie_arena, int32_t *status,
                                         void *stream)
{
    if (!ctx || (n && (!items || !id_arena || !cookie_arena || !status))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (n == 0) return 0;
    return cookie_launch(CK_WRITE, ctx, now, items, n, nullptr, id_arena, cookie_arena, status, true,
                         (hipStream_t) stream);
}

extern "C" int tlsrec_cookie_batch_check(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_cookie_item *items,
                                         uint32_t n, const uint8_t *id_arena, const uint8_t *cookie_arena,
                                         int32_t *status, void *stream)
{
    if (!ctx || (n && (!items || !id_arena || !cookie_arena || !status))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (n == 0) return 0;
    return cookie_launch(CK_CHECK, ctx, now, items, n, cookie_arena, id_arena, nullptr, status, true,
                         (hipStream_t) stream);
}

extern "C" int tlsrec_dtls_check_clihlo_cookies(const tlsrec_cookie_ctx *ctx, uint64_t now, const tlsrec_clihlo *hellos,
                                                uint32_t n, const uint8_t *arena, const uint8_t *id_arena,
                                                uint8_t *out_arena, tlsrec_clihlo_res *res, void *stream)
{
    if (!ctx || (n && (!hellos || !arena || !id_arena || !out_arena || !res))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (n == 0) return 0;
    return cookie_launch(CK_HELLO, ctx, now, hellos, n, arena, id_arena, out_arena, &res->status, true,
                         (hipStream_t) stream);
}

/* One client in host buffers: a batch of one staged in the single-shot arena
 * (item at 0, status at 32, cookie at 64, id at 96). */
static int cookie_single(int mode, tlsrec_cookie_ctx *ctx, unsigned char *cookie, size_t cookie_len,
                         const unsigned char *cli_id, size_t cli_id_len)
{
    enum { AT_STATUS = 32, AT_COOKIE = 64, AT_ID = 96, BYTES = 96 + 256 };
    uint8_t h[BYTES];
    memset(h, 0, sizeof(h));
    tlsrec_cookie_item it;
    it.id_off = AT_ID;
    it.cookie_off = AT_COOKIE;
    it.id_len = cli_id_len > 255 ? 256u : (uint32_t) cli_id_len;
    it.cookie_len = cookie_len > 0xffffffffu ? 0xffffffffu : (uint32_t) cookie_len;
    memcpy(h, &it, sizeof(it));
    const int32_t unreached = TLSREC_ERR_SSL_INTERNAL_ERROR;
    memcpy(h + AT_STATUS, &unreached, 4);
    if (mode == CK_CHECK && cookie_len == TLSREC_COOKIE_LEN) memcpy(h + AT_COOKIE, cookie, TLSREC_COOKIE_LEN);
    if (it.id_len <= 255) memcpy(h + AT_ID, cli_id, it.id_len);
    const uint64_t now = (uint64_t) time(nullptr);
    uint8_t *dev;
    hipStream_t ks;
    int r = tlsrec_ks_arena_lock(&dev, &ks);
    if (r == 0) {
        hipError_t e = hipMemcpyAsync(dev, h, BYTES, hipMemcpyHostToDevice, ks);
        if (e == hipSuccess &&
            cookie_launch(mode, ctx, now, dev, 1, dev, dev, dev, (int32_t *) (dev + AT_STATUS), false, ks) != 0)
            e = hipErrorLaunchFailure;
        if (e == hipSuccess) e = hipMemcpyAsync(h + AT_STATUS, dev + AT_STATUS, AT_ID - AT_STATUS, hipMemcpyDeviceToHost, ks);
        if (e == hipSuccess) e = hipStreamSynchronize(ks);
        if (e != hipSuccess) r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
        tlsrec_ks_arena_unlock();
    }
    if (r == 0) {
        int32_t st;
        memcpy(&st, h + AT_STATUS, 4);
        r = st;
        if (mode == CK_WRITE && st == 0) memcpy(cookie, h + AT_COOKIE, TLSREC_COOKIE_LEN);
    }
    return r;
}

extern "C" int tlsrec_cookie_write(void *ctx, unsigned char **p, unsigned char *end, const unsigned char *cli_id,
                                   size_t cli_id_len)
{
    if (!ctx || !cli_id || !p || !*p) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    const size_t space = end > *p ? (size_t) (end - *p) : 0;
    const int r = cookie_single(CK_WRITE, (tlsrec_cookie_ctx *) ctx, *p, space, cli_id, cli_id_len);
    if (r == 0) *p += TLSREC_COOKIE_LEN;
    return r;
}

extern "C" int tlsrec_cookie_check(void *ctx, const unsigned char *cookie, size_t cookie_len, const unsigned char *cli_id,
                                   size_t cli_id_len)
{
    if (!ctx || !cli_id || (!cookie && cookie_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return cookie_single(CK_CHECK, (tlsrec_cookie_ctx *) ctx, (unsigned char *) cookie, cookie_len, cli_id, cli_id_len);
}
