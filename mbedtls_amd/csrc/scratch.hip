/*
 * scratch.hip -- per-(device, stream, kind) device scratch, reused across calls (tlsrec_internal.h): the
 * bucket pass's arrays and the stream record layer's staging.
 */
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

#include "tlsrec.h"
#include "tlsrec_internal.h"

struct ScratchEntry {
    int device;
    hipStream_t stream;
    uintptr_t thread;         /* hipStreamPerThread: the calling thread (its own real stream) */
    int kind;
    void *mem;
    size_t bytes;
    pthread_mutex_t mu;
    ScratchEntry *next;
};
static pthread_mutex_t g_scratch_mu = PTHREAD_MUTEX_INITIALIZER;
static ScratchEntry *g_scratch = nullptr;

/* hipStreamPerThread entries belong to their thread: when it exits they are
 * marked orphaned, and the next acquire frees them, so a server whose
 * connections come and go on short-lived threads does not accumulate device
 * memory.  The exit hook itself makes no HIP call: it runs after
 * the HIP runtime's own thread-local state is gone.  hipFree waits for the
 * device, so work the dead thread left on its stream has finished by then. */
static const uintptr_t SCRATCH_ORPHAN = 1;     /* never a pthread_t of a live thread */
static pthread_key_t g_scratch_key;
static pthread_once_t g_scratch_once = PTHREAD_ONCE_INIT;
static volatile int g_scratch_orphans = 0;

static void scratch_thread_exit(void *)
{
    const uintptr_t me = (uintptr_t) pthread_self();
    pthread_mutex_lock(&g_scratch_mu);
    for (ScratchEntry *e = g_scratch; e; e = e->next)
        if (e->thread == me) {
            e->thread = SCRATCH_ORPHAN;
            g_scratch_orphans++;
        }
    pthread_mutex_unlock(&g_scratch_mu);
}

static void scratch_key_init(void) { pthread_key_create(&g_scratch_key, scratch_thread_exit); }

/* Under g_scratch_mu: unlink the orphaned entries (their threads exited) and
 * return them as a list; scratch_free_list frees them after the lock is
 * dropped -- hipFree waits for the device (a record-server grid, other
 * streams' kernels), and no other launcher should queue behind that. */
static ScratchEntry *scratch_reclaim_locked(void)
{
    ScratchEntry *dead = nullptr;
    for (ScratchEntry **pp = &g_scratch; *pp;) {
        ScratchEntry *e = *pp;
        if (e->thread == SCRATCH_ORPHAN) {
            *pp = e->next;
            e->next = dead;
            dead = e;
            g_scratch_orphans--;
        } else {
            pp = &e->next;
        }
    }
    return dead;
}

static void scratch_free_list(ScratchEntry *e)
{
    while (e) {
        ScratchEntry *next = e->next;
        if (e->mem) (void) hipFree(e->mem);
        pthread_mutex_destroy(&e->mu);
        free(e);
        e = next;
    }
}

extern "C" int tlsrec__scratch_acquire(hipStream_t st, int kind, size_t bytes, tlsrec_scratch_lease *lease)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    /* one handle, one ordered queue -- except hipStreamPerThread, which names
     * a different real stream in every thread: two threads' batches on it run
     * unordered on the GPU, so each thread gets its own scratch (the null
     * stream is one queue for every thread and needs nothing) */
    const uintptr_t thr = st == hipStreamPerThread ? (uintptr_t) pthread_self() : 0;
    pthread_mutex_lock(&g_scratch_mu);
    ScratchEntry *dead = g_scratch_orphans ? scratch_reclaim_locked() : nullptr;
    ScratchEntry *e = g_scratch;
    while (e && !(e->device == dev && e->stream == st && e->thread == thr && e->kind == kind)) e = e->next;
    if (!e) {
        e = (ScratchEntry *) calloc(1, sizeof(*e));
        if (!e) {
            pthread_mutex_unlock(&g_scratch_mu);
            scratch_free_list(dead);
            return TLSREC_ERR_SSL_ALLOC_FAILED;
        }
        e->device = dev;
        e->stream = st;
        e->thread = thr;
        e->kind = kind;
        pthread_mutex_init(&e->mu, NULL);
        e->next = g_scratch;
        g_scratch = e;
        if (thr) {
            pthread_once(&g_scratch_once, scratch_key_init);
            pthread_setspecific(g_scratch_key, (void *) 1);   /* non-NULL: the destructor runs */
        }
    }
    pthread_mutex_unlock(&g_scratch_mu);
    scratch_free_list(dead);
    pthread_mutex_lock(&e->mu);
    if (e->bytes < bytes) {
        /* grow: the stream's earlier work may still read the old buffer */
        if (e->mem && (hipStreamSynchronize(st) != hipSuccess || hipFree(e->mem) != hipSuccess)) {
            pthread_mutex_unlock(&e->mu);
            return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
        }
        e->mem = nullptr;
        e->bytes = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipMalloc(&e->mem, want) != hipSuccess) {
            e->mem = nullptr;
            pthread_mutex_unlock(&e->mu);
            return TLSREC_ERR_SSL_ALLOC_FAILED;
        }
        e->bytes = want;
    }
    lease->mem = e->mem;
    lease->entry = e;
    return 0;
}

/* diagnostics (tests): scratch entries alive, and their device bytes */
extern "C" uint32_t tlsrec__scratch_entries(uint64_t *bytes)
{
    uint32_t n = 0;
    uint64_t b = 0;
    pthread_mutex_lock(&g_scratch_mu);
    for (ScratchEntry *e = g_scratch; e; e = e->next) {
        n++;
        b += e->bytes;
    }
    pthread_mutex_unlock(&g_scratch_mu);
    if (bytes) *bytes = b;
    return n;
}

extern "C" void tlsrec__scratch_release(tlsrec_scratch_lease *lease)
{
    if (lease && lease->entry) {
        pthread_mutex_unlock(&((ScratchEntry *) lease->entry)->mu);
        lease->entry = nullptr;
        lease->mem = nullptr;
    }
}
