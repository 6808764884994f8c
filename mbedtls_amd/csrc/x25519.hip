/*
 * x25519.hip -- X25519 key shares and shared secrets on the GPU, in batches
 * (tlsrec_x25519_batch_public, tlsrec_x25519_batch_shared).
 *
 *   reference                                                    here
 *   psa_generate_key + psa_export_public_key
 *                          ssl_tls13_generic.c:1566-1582         x25519_kernel<true>
 *   psa_raw_key_agreement  ssl_tls13_keys.c:1457,
 *                          ssl_tls12_server.c:2603-2631, :3028   x25519_kernel<false>
 *
 * One connection per lane, 64 lanes per workgroup, no LDS, like the ladders of
 * tls13_ladder.hip.  The arithmetic is tlsrec_x25519.h, the same body the host
 * export tlsrec__x25519_host runs for the CPU tests.  A lane loads its scalar
 * (and the peer's u-coordinate) as eight words, runs the ladder and stores 32
 * bytes: 16-byte accesses where pointer and stride are 16-byte aligned, bytes
 * otherwise (the convention of tls12_load_conn).
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tlsrec.h"
#include "tlsrec_x25519.h"

namespace tlsks {

struct X25519Args {
    const uint8_t *priv;
    const uint8_t *peer;
    uint8_t *out;
    uint32_t *ok;
    uint32_t peer_stride, out_stride, count;
    uint32_t priv_aligned, peer_aligned, out_aligned;
};

__device__ __forceinline__ void x_load32(const uint8_t *p, bool aligned, uint32_t (&w)[8])
{
    if (aligned) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
        const uint4 a = q[0], b = q[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            w[j] = (uint32_t) p[4 * j] | ((uint32_t) p[4 * j + 1] << 8) | ((uint32_t) p[4 * j + 2] << 16) |
                   ((uint32_t) p[4 * j + 3] << 24);
    }
}

__device__ __forceinline__ void x_store32(uint8_t *p, bool aligned, const uint32_t (&w)[8])
{
    if (aligned) {
        uint4 *q = reinterpret_cast<uint4 *>(p);
        q[0] = make_uint4(w[0], w[1], w[2], w[3]);
        q[1] = make_uint4(w[4], w[5], w[6], w[7]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int b = 0; b < 4; b++) p[4 * j + b] = (uint8_t) (w[j] >> (8 * b));
        }
    }
}

/* BASE: the public share X25519(priv, 9); otherwise the agreement with the peer's share and ok[i] */
template <bool BASE> __global__ void __launch_bounds__(64) x25519_kernel(X25519Args a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    uint32_t k[8], u[8], r[8];
    x_load32(a.priv + 32 * (size_t) i, a.priv_aligned != 0, k);
    if constexpr (BASE) {
#pragma unroll
        for (int j = 0; j < 8; j++) u[j] = 0;
    } else {
        x_load32(a.peer + (size_t) a.peer_stride * i, a.peer_aligned != 0, u);
    }
    const uint32_t ok = tlsrec::x25519<BASE>(r, k, u);
    x_store32(a.out + (size_t) a.out_stride * i, a.out_aligned != 0, r);
    if constexpr (!BASE) a.ok[i] = ok;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        k[j] = 0;
        r[j] = 0;
    }
}

static bool x_aligned(const void *p, uint32_t stride) { return ((((uintptr_t) p) | stride) & 15) == 0; }

template <bool BASE> static int x25519_launch(const X25519Args &a, void *stream)
{
    static const int device = tlsrec_device_check();     /* no key table vouches for a device here; asked once */
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    const dim3 grid((a.count + 63) / 64), block(64);
    hipLaunchKernelGGL(x25519_kernel<BASE>, grid, block, 0, (hipStream_t) stream, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

}  // namespace tlsks

using namespace tlsks;

extern "C" int tlsrec_x25519_batch_public(const uint8_t *priv, uint8_t *pub, uint32_t pub_stride, uint32_t count,
                                          void *stream)
{
    if ((!priv || !pub) && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (pub_stride < 32) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    X25519Args a;
    a.priv = priv;
    a.peer = nullptr;
    a.out = pub;
    a.ok = nullptr;
    a.peer_stride = 0;
    a.out_stride = pub_stride;
    a.count = count;
    a.priv_aligned = x_aligned(priv, 32);
    a.peer_aligned = 0;
    a.out_aligned = x_aligned(pub, pub_stride);
    return x25519_launch<true>(a, stream);
}

extern "C" int tlsrec_x25519_batch_shared(const uint8_t *priv, const uint8_t *peer, uint32_t peer_stride, uint8_t *out,
                                          uint32_t out_stride, uint32_t *ok, uint32_t count, void *stream)
{
    if ((!priv || !peer || !out || !ok) && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (peer_stride < 32 || out_stride < 32) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    X25519Args a;
    a.priv = priv;
    a.peer = peer;
    a.out = out;
    a.ok = ok;
    a.peer_stride = peer_stride;
    a.out_stride = out_stride;
    a.count = count;
    a.priv_aligned = x_aligned(priv, 32);
    a.peer_aligned = x_aligned(peer, peer_stride);
    a.out_aligned = x_aligned(out, out_stride);
    return x25519_launch<false>(a, stream);
}

/* The header's ladder on the CPU, for the CPU tests only (no fallback: the public calls stay
 * GPU-only).  Returns the ok flag. */
extern "C" int tlsrec__x25519_host(uint8_t out[32], const uint8_t scalar[32], const uint8_t point[32])
{
    uint32_t k[8], u[8], r[8];
    for (int j = 0; j < 8; j++) {
        k[j] = (uint32_t) scalar[4 * j] | ((uint32_t) scalar[4 * j + 1] << 8) | ((uint32_t) scalar[4 * j + 2] << 16) |
               ((uint32_t) scalar[4 * j + 3] << 24);
        u[j] = (uint32_t) point[4 * j] | ((uint32_t) point[4 * j + 1] << 8) | ((uint32_t) point[4 * j + 2] << 16) |
               ((uint32_t) point[4 * j + 3] << 24);
    }
    const uint32_t ok = tlsrec::x25519<false>(r, k, u);
    for (int j = 0; j < 32; j++) out[j] = (uint8_t) (r[j >> 2] >> (8 * (j & 3)));
    for (int j = 0; j < 8; j++) k[j] = r[j] = 0;
    return (int) ok;
}
