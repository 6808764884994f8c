/*
 * host_pipe.hip -- records in host memory: chunked H2D -> kernel -> D2H pipeline
 * (tlsrec_host_batch_*).  Records start and end in host socket buffers
 * (SURVEY.md 8(d)); a chunk is a run of consecutive records, its byte range
 * [buf_off of the first, end of the last) goes to one of NSLOT device slots,
 * is protected there in place, and comes back to the same offsets of the
 * output arena.  Three streams (H2D, kernels, D2H) chained by events keep
 * both copy directions and the kernels busy at once.
 */
#include <hip/hip_runtime.h>
#include <new>
#include <stdint.h>
#include <stdlib.h>

#include "tlsrec.h"
#include "tlsrec_internal.h"

using namespace tlsrec;

static constexpr int PIPE_SLOTS = 3;

struct HostPipe {
    hipStream_t h2d, cmp, d2h;
    hipEvent_t ev_h2d[PIPE_SLOTS], ev_cmp[PIPE_SLOTS], ev_d2h[PIPE_SLOTS];
    uint8_t *slot[PIPE_SLOTS];
    size_t slot_bytes;
    tlsrec_batch_rec *d_recs;
    tlsrec_batch_res *d_res;
    size_t nrec_cap;
};

void tlsrec__host_pipe_free(HostPipe *p)
{
    if (!p) return;
    if (p->h2d) hipStreamSynchronize(p->h2d);
    if (p->cmp) hipStreamSynchronize(p->cmp);
    if (p->d2h) hipStreamSynchronize(p->d2h);
    for (int i = 0; i < PIPE_SLOTS; i++) {
        hipFree(p->slot[i]);
        if (p->ev_h2d[i]) hipEventDestroy(p->ev_h2d[i]);
        if (p->ev_cmp[i]) hipEventDestroy(p->ev_cmp[i]);
        if (p->ev_d2h[i]) hipEventDestroy(p->ev_d2h[i]);
    }
    hipFree(p->d_recs);
    hipFree(p->d_res);
    if (p->h2d) hipStreamDestroy(p->h2d);
    if (p->cmp) hipStreamDestroy(p->cmp);
    if (p->d2h) hipStreamDestroy(p->d2h);
    delete p;
}

/* *pp: the table's pipeline (tlsrec__keytab_pipe_lock), made here on first use */
static int host_pipe_reserve(HostPipe **pp, size_t slot_bytes, size_t nrec)
{
    HostPipe *p = *pp;
    if (!p) {
        p = new (std::nothrow) HostPipe();
        if (!p) return TLSREC_ERR_SSL_ALLOC_FAILED;
        *pp = p;
        if (hipStreamCreateWithFlags(&p->h2d, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&p->cmp, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&p->d2h, hipStreamNonBlocking) != hipSuccess)
            return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
        for (int i = 0; i < PIPE_SLOTS; i++)
            if (hipEventCreateWithFlags(&p->ev_h2d[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&p->ev_cmp[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&p->ev_d2h[i], hipEventDisableTiming) != hipSuccess)
                return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    if (p->slot_bytes < slot_bytes) {
        for (int i = 0; i < PIPE_SLOTS; i++) {
            hipFree(p->slot[i]);
            p->slot[i] = NULL;
        }
        p->slot_bytes = 0;
        for (int i = 0; i < PIPE_SLOTS; i++)
            if (hipMalloc((void **) &p->slot[i], slot_bytes) != hipSuccess) return TLSREC_ERR_SSL_ALLOC_FAILED;
        p->slot_bytes = slot_bytes;
    }
    if (p->nrec_cap < nrec) {
        hipFree(p->d_recs);
        hipFree(p->d_res);
        p->d_recs = NULL;
        p->d_res = NULL;
        p->nrec_cap = 0;
        if (hipMalloc((void **) &p->d_recs, nrec * sizeof(tlsrec_batch_rec)) != hipSuccess ||
            hipMalloc((void **) &p->d_res, nrec * sizeof(tlsrec_batch_res)) != hipSuccess)
            return TLSREC_ERR_SSL_ALLOC_FAILED;
        p->nrec_cap = nrec;
    }
    return 0;
}

static int host_batch(tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res, uint32_t n,
                      const uint8_t *in, uint8_t *out, uint32_t lanes, uint64_t chunk_bytes, int dec)
{
    if (!kt || (n && (!recs || !res || !in || !out))) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (n == 0) return 0;
    if (chunk_bytes == 0) chunk_bytes = 64ull << 20;   /* measured best of 16 / 64 / 256 / 1024 MiB */
    /* records in ascending, non-overlapping order; chunks of whole records */
    struct Chunk { uint32_t first, count; uint64_t base, span; };
    Chunk *ch = (Chunk *) malloc(sizeof(Chunk) * n);
    if (!ch) return TLSREC_ERR_SSL_ALLOC_FAILED;
    uint32_t nch = 0;
    uint64_t maxspan = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t lo = recs[i].buf_off, hi = lo + recs[i].buf_len;
        if (i && lo < recs[i - 1].buf_off + recs[i - 1].buf_len) {
            free(ch);
            return TLSREC_ERR_SSL_BAD_INPUT_DATA;
        }
        if (nch && hi - ch[nch - 1].base <= chunk_bytes) {
            ch[nch - 1].count++;
            ch[nch - 1].span = hi - ch[nch - 1].base;
        } else {
            ch[nch++] = Chunk{ i, 1, lo, hi - lo };
        }
        if (ch[nch - 1].span > maxspan) maxspan = ch[nch - 1].span;
    }
    /* Output arena in pinned host memory the device can address: the kernels
     * write their output straight into it over PCIe (measured 48-49 GiB/s
     * for c2-shaped records, the link rate) while the next chunk's H2D copy
     * runs on the copy engine -- a D2H copy instead shares that engine with
     * the H2D copies and the two directions serialise.  Pageable output:
     * protect in place in the device slot and copy the chunk back. */
    uint8_t *zc = NULL;
    {
        hipPointerAttribute_t at;
        const char *zce = getenv("TLSREC_HOST_ZC");      /* =0: copy back even to pinned memory (measurement) */
        if (!(zce && atoi(zce) == 0) && hipPointerGetAttributes(&at, out) == hipSuccess && at.type == hipMemoryTypeHost &&
            at.devicePointer)
            zc = (uint8_t *) at.devicePointer;
        else
            (void) hipGetLastError();    /* pageable memory: clear the sticky error */
    }
    HostPipe **pp = tlsrec__keytab_pipe_lock(kt);
    int rc = host_pipe_reserve(pp, align_up(maxspan, 256), n);
    HostPipe *p = *pp;
    if (!rc && hipMemcpyAsync(p->d_recs, recs, (size_t) n * sizeof(*recs), hipMemcpyHostToDevice, p->cmp) != hipSuccess)
        rc = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    for (uint32_t c = 0; c < nch && !rc; c++) {
        const int k = (int) (c % PIPE_SLOTS);
        const Chunk &C = ch[c];
        hipError_t e = hipSuccess;
        if (c >= PIPE_SLOTS) e = hipStreamWaitEvent(p->h2d, p->ev_d2h[k], 0);      /* slot drained */
        if (e == hipSuccess) e = hipMemcpyAsync(p->slot[k], in + C.base, C.span, hipMemcpyHostToDevice, p->h2d);
        if (e == hipSuccess) e = hipEventRecord(p->ev_h2d[k], p->h2d);
        if (e == hipSuccess) e = hipStreamWaitEvent(p->cmp, p->ev_h2d[k], 0);
        if (e != hipSuccess) {
            rc = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
            break;
        }
        /* the descriptors' buf_off are offsets into the host arena: shift the
         * device arena base so that base + buf_off lands in the slot */
        uint8_t *dev = (uint8_t *) ((uintptr_t) p->slot[k] - (uintptr_t) C.base);
        BatchOpt o;
        o.avg_bytes = (uint32_t) (C.span / (C.count ? C.count : 1));
        rc = batch(kt, p->d_recs + C.first, p->d_res + C.first, C.count, dev, zc ? zc : dev, lanes, p->cmp, dec, o);
        if (rc) break;
        e = hipEventRecord(p->ev_cmp[k], p->cmp);
        /* the slot is free once its kernel is done (zero-copy) or its chunk has been copied back */
        if (e == hipSuccess) e = hipStreamWaitEvent(p->d2h, p->ev_cmp[k], 0);
        if (e == hipSuccess && !zc)
            e = hipMemcpyAsync(out + C.base, p->slot[k], C.span, hipMemcpyDeviceToHost, p->d2h);
        if (e == hipSuccess) e = hipEventRecord(p->ev_d2h[k], p->d2h);
        if (e != hipSuccess) rc = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    if (!rc && (hipStreamSynchronize(p->cmp) != hipSuccess ||
                hipMemcpyAsync(res, p->d_res, (size_t) n * sizeof(*res), hipMemcpyDeviceToHost, p->d2h) != hipSuccess))
        rc = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    if (p) {
        /* drain every stream before the caller may reuse its buffers */
        if (hipStreamSynchronize(p->h2d) != hipSuccess || hipStreamSynchronize(p->cmp) != hipSuccess ||
            hipStreamSynchronize(p->d2h) != hipSuccess)
            rc = rc ? rc : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    tlsrec__keytab_pipe_unlock(kt);
    free(ch);
    return rc;
}

extern "C" int tlsrec_host_batch_encrypt(tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                                         uint32_t n, const uint8_t *in_arena, uint8_t *out_arena,
                                         uint32_t lanes_per_record, uint64_t chunk_bytes)
{
    return host_batch(kt, recs, res, n, in_arena, out_arena, lanes_per_record, chunk_bytes, 0);
}

extern "C" int tlsrec_host_batch_decrypt(tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                                         uint32_t n, const uint8_t *in_arena, uint8_t *out_arena,
                                         uint32_t lanes_per_record, uint64_t chunk_bytes)
{
    return host_batch(kt, recs, res, n, in_arena, out_arena, lanes_per_record, chunk_bytes, 1);
}
