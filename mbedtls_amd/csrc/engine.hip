/*
 * engine.hip -- the engine of the single-record API (tlsrec_host.c).  Plain HIP
 * runtime C++, no CPU crypto: a record is only ever transformed by the kernels.
 *
 * Key slots live in pages of ENGINE_PAGE_SLOTS (one key table each), added
 * as connections arrive -- ENGINE_MAX_PAGES x 4096 = 1 M slots, i.e. 512 K
 * connections per process.
 *
 * Concurrent calls are coalesced (flat combining, per page): a call queues
 * its record; if fewer than ENGINE_SETS batches of the page are in flight it
 * becomes the leader of the next one, takes every queued record (up to
 * ENGINE_BATCH, either direction), stages them in one pinned buffer, and runs
 * one H2D copy, one launch per direction and cipher (batch.hip, identity
 * order: no bucket pass), one D2H copy and one sync for all of them; the
 * callers whose records it carried are woken with their results.  A lone call
 * is its own leader: one record, one round trip.  Under load a round trip
 * carries as many records as arrived during the previous one.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_cbc.h"
#include "tlsrec_frame.h"
#include "tlsrec_internal.h"

using namespace tlsrec;

#define ENGINE_PAGE_SLOTS 4096
#define ENGINE_MAX_PAGES 256
#define ENGINE_SETS 2                    /* batches of a queue in flight at once (own streams) */
#define ENGINE_BATCH 256                 /* records per coalesced batch */
#define ENGINE_ALIGN 128                 /* record slots in the staging arena */

struct EngineReq {
    int dec;
    tlsrec_batch_rec d;                  /* slot = page-local */
    uint32_t cipher;
    unsigned char *buf;
    size_t buf_len;
    const unsigned char *cid;
    tlsrec_batch_res res;
    int rc;
    int done;                            /* guarded by the combiner's mutex */
    EngineReq *next;
};

/* one staging set: [descriptors][results][arena], pinned host memory the
 * device can address (hd = its device address), and a device copy */
struct EngineSet {
    hipStream_t st;
    uint8_t *h, *hd, *d;
    size_t cap;
    int busy;
};

/* Batches up to this many staged bytes run zero-copy: the kernels read the
 * records from, and write them back to, the pinned staging area over PCIe
 * (no copy-engine round trips: measured on MI355X, an H2D or D2H copy of a
 * small record costs ~12 us with its sync, a whole kernel launch ~10 us,
 * tools/probes/latency_probe.hip).  TLSREC_ENGINE_ZC=0 stages through device
 * memory always; =<bytes> moves the bound. */
static size_t engine_zc_max(void)
{
    static size_t v = (size_t) -1;
    if (v == (size_t) -1) {
        const char *e = getenv("TLSREC_ENGINE_ZC");
        v = e ? (size_t) strtoull(e, NULL, 0) : (size_t) (64u << 10);
    }
    return v;
}

struct Combiner {
    pthread_mutex_t mu;
    pthread_cond_t cv;
    EngineReq *head, *tail;
    EngineSet set[ENGINE_SETS];
    uint64_t batches, records;           /* statistics (tlsrec__engine_stats) */
};

/* A page queues records per (AEAD family, direction): each batch is then one
 * kernel launch, and a call never waits behind another family's kernel --
 * CCM's CBC-MAC is one dependent AES chain per record (a 1.4 KiB record is
 * ~170 us on one lane), GCM and ChaCha20-Poly1305 records take ~25 us.  CBC +
 * HMAC is a family of its own for the same reason: its hash, and on encrypt
 * its cipher too, is hundreds of microseconds of dependent work per record. */
#define ENGINE_QUEUES 8
static int engine_queue(uint32_t cipher, int dec)
{
    const int fam = cipher == TLSREC_CIPHER_CHACHA20_POLY1305 ? 1
                    : (tlsrec_cipher_is_ccm((int) cipher) || tlsrec_cipher_is_alt_ccm((int) cipher)) ? 2
                    : cbc_is_cipher((int) cipher) ? 3 : 0;
    return fam * 2 + (dec ? 1 : 0);
}

struct EnginePage {
    tlsrec_keytab *kt;
    uint8_t used[ENGINE_PAGE_SLOTS];
    uint8_t cid[ENGINE_PAGE_SLOTS];      /* the slot has a DTLS connection ID (the record server takes none) */
    uint8_t etm[ENGINE_PAGE_SLOTS];      /* a CBC slot's MAC order: 1 = encrypt-then-MAC (tlsrec__engine_slot_mac_order) */
    uint32_t nused;
    Combiner *co[ENGINE_QUEUES];
};

static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;   /* slot allocation, page growth */
static EnginePage g_pages[ENGINE_MAX_PAGES];
static volatile int g_npages = 0;
static hipStream_t g_load = NULL;
static volatile int g_ready = 0;

static int engine_init_locked(void)
{
    if (g_ready) return 0;
    if (tlsrec_device_check() != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    if (hipStreamCreateWithFlags(&g_load, hipStreamNonBlocking) != hipSuccess) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    g_ready = 1;
    return 0;
}

static void combiner_free(Combiner *c)
{
    if (!c) return;
    for (int i = 0; i < ENGINE_SETS; i++) {
        if (c->set[i].st) {
            hipStreamSynchronize(c->set[i].st);
            hipStreamDestroy(c->set[i].st);
        }
        if (c->set[i].h) hipHostFree(c->set[i].h);
        if (c->set[i].d) hipFree(c->set[i].d);
    }
    pthread_cond_destroy(&c->cv);
    pthread_mutex_destroy(&c->mu);
    free(c);
}

static Combiner *combiner_new(void)
{
    Combiner *c = (Combiner *) calloc(1, sizeof(Combiner));
    if (!c) return NULL;
    pthread_mutex_init(&c->mu, NULL);
    pthread_cond_init(&c->cv, NULL);
    for (int i = 0; i < ENGINE_SETS; i++)
        if (hipStreamCreateWithFlags(&c->set[i].st, hipStreamNonBlocking) != hipSuccess) {
            c->set[i].st = NULL;
            combiner_free(c);      /* the streams created before this one */
            return NULL;
        }
    return c;
}

static tlsrec_keytab *slot_table(int slot, uint32_t *idx)
{
    if (slot < 0) return NULL;
    const int pg = slot / ENGINE_PAGE_SLOTS;
    if (pg >= g_npages) return NULL;
    *idx = (uint32_t) (slot % ENGINE_PAGE_SLOTS);
    return g_pages[pg].kt;
}

/* A free slot of some page (a new page when every one is full), loaded with km, or with the CBC material ck
 * when km is NULL */
static int engine_slot_alloc(const tlsrec_key_material *km, const tlsrec_cbc_key_material *ck)
{
    pthread_mutex_lock(&g_mu);
    int r = engine_init_locked();
    int slot = -1;
    int pg = 0;
    if (r == 0) {
        for (pg = 0; pg < g_npages; pg++)
            if (g_pages[pg].nused < ENGINE_PAGE_SLOTS) break;
        if (pg == g_npages) {
            if (pg == ENGINE_MAX_PAGES) {
                r = TLSREC_ERR_SSL_ALLOC_FAILED;
            } else {
                EnginePage &N = g_pages[pg];
                r = tlsrec_keytab_create(&N.kt, ENGINE_PAGE_SLOTS);
                for (int q = 0; r == 0 && q < ENGINE_QUEUES; q++)
                    if (!(N.co[q] = combiner_new())) r = TLSREC_ERR_SSL_ALLOC_FAILED;
                if (r != 0) {
                    /* unwind the partial page: nothing of it stays allocated or pointed at */
                    for (int q = 0; q < ENGINE_QUEUES; q++) {
                        combiner_free(N.co[q]);
                        N.co[q] = NULL;
                    }
                    if (N.kt) tlsrec_keytab_free(N.kt);
                    N.kt = NULL;
                }
                if (r == 0) g_npages = pg + 1;
            }
        }
    }
    if (r == 0) {
        EnginePage &P = g_pages[pg];
        for (int i = 0; i < ENGINE_PAGE_SLOTS; i++)
            if (!P.used[i]) { slot = i; break; }
        r = km ? tlsrec_keytab_load(P.kt, (uint32_t) slot, 1, km, 0, g_load)
               : tlsrec_keytab_load_cbc(P.kt, (uint32_t) slot, 1, ck, 0, g_load);
        if (r == 0 && hipStreamSynchronize(g_load) != hipSuccess) r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
        if (r == 0) {
            P.used[slot] = 1;
            P.cid[slot] = 0;
            P.etm[slot] = km ? 0 : ck->etm;
            P.nused++;
            slot += pg * ENGINE_PAGE_SLOTS;
        }
    }
    pthread_mutex_unlock(&g_mu);
    return r ? r : slot;
}

extern "C" int tlsrec__engine_slot_alloc(const tlsrec_key_material *km) { return engine_slot_alloc(km, NULL); }

/* The same for a CBC + HMAC slot (tlsrec_transform_setup_cbc).  tlsrec_keytab_load_cbc stages the material in
 * a device buffer of its own and zeroizes it once the key setup has run: the raw MAC key stays nowhere. */
extern "C" int tlsrec__engine_slot_alloc_cbc(const tlsrec_cbc_key_material *ck)
{
    return ck ? engine_slot_alloc(NULL, ck) : TLSREC_ERR_SSL_BAD_INPUT_DATA;
}

/* a CBC slot's MAC order: 0 = MAC-then-encrypt, 1 = encrypt-then-MAC; -1 for no slot in use */
extern "C" int tlsrec__engine_slot_mac_order(int slot)
{
    pthread_mutex_lock(&g_mu);
    uint32_t i = 0;
    const int r = slot_table(slot, &i) && g_pages[slot / ENGINE_PAGE_SLOTS].used[i]
                      ? g_pages[slot / ENGINE_PAGE_SLOTS].etm[i] : -1;
    pthread_mutex_unlock(&g_mu);
    return r;
}

extern "C" void tlsrec__engine_slot_free(int slot)
{
    pthread_mutex_lock(&g_mu);
    uint32_t i = 0;
    tlsrec_keytab *kt = slot_table(slot, &i);
    EnginePage *P = kt ? &g_pages[slot / ENGINE_PAGE_SLOTS] : NULL;
    if (kt && P->used[i]) {
        tlsrec__keytab_slot_zeroize(kt, i, g_load);
        P->used[i] = 0;
        P->etm[i] = 0;
        P->nused--;
    }
    pthread_mutex_unlock(&g_mu);
}

#ifdef TLSREC_TEST_HOOKS
/* Test hooks (the test build only; tlsrec__test_skip_record and the launch log: batch.hip):
 *   tlsrec__test_fail_staging  the next n staging-area allocations of the
 *                              single-record engine fail (ALLOC_FAILED path)
 *   tlsrec__test_server_shadow served records read their key state from
 *                              copies at addresses whose low 32 bits have bit
 *                              31 set (the readfirstlane sign-extension case) */
static volatile int g_test_fail_staging = 0;
static uint8_t *g_test_shadow = nullptr;
static size_t g_test_shadow_bytes = 0;

extern "C" void tlsrec__test_fail_staging(int n) { g_test_fail_staging = n; }
extern "C" void tlsrec__test_server_shadow(void *dev, size_t bytes)
{
    g_test_shadow = (uint8_t *) dev;
    g_test_shadow_bytes = dev ? bytes : 0;
}

/*   tlsrec__test_engine_slot_dump  the device bytes of an engine slot -- its SlotState (1024 B),
 * the first 1024 B of its GHASH tables and its 64 record-server powers
 * (1024 B) -- copied to host, to show what slot_free leaves behind */
extern "C" int tlsrec__test_engine_slot_dump(int slot, void *state, void *ghtab, void *hpw)
{
    pthread_mutex_lock(&g_mu);
    uint32_t i = 0;
    tlsrec_keytab *kt = slot_table(slot, &i);
    int r = kt ? 0 : TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!r) {
        const uint4 *tab = tlsrec__keytab_ghtab(kt) + (size_t) i * KEY_TABLE_WORDS;
        if (hipMemcpy(state, tlsrec__keytab_slots(kt) + i, sizeof(SlotState), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ghtab, tab, 1024, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hpw, tab + KEY_HPOW_OFF, 1024, hipMemcpyDeviceToHost) != hipSuccess)
            r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    pthread_mutex_unlock(&g_mu);
    return r;
}
#endif

extern "C" int tlsrec__engine_slot_set_cid(int slot, const unsigned char *cid, size_t cid_len)
{
    pthread_mutex_lock(&g_mu);
    uint32_t i = 0;
    tlsrec_keytab *kt = slot_table(slot, &i);
    int r = kt && g_pages[slot / ENGINE_PAGE_SLOTS].used[i] ? tlsrec_keytab_set_cid(kt, i, cid, cid_len, g_load)
                                                            : TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (r == 0) g_pages[slot / ENGINE_PAGE_SLOTS].cid[i] = cid_len != 0;
    pthread_mutex_unlock(&g_mu);
    return r;
}

/* Leader: stage `n` records (linked from `first`), run them, fill in their
 * results.  Records of one direction are contiguous in the staging area
 * (encrypt first), each in its own ENGINE_ALIGN-aligned arena slot with its
 * CID bytes behind the buffer. */
static int run_batch(tlsrec_keytab *kt, EngineSet &S, EngineReq *first, uint32_t n)
{
    EngineReq *v[ENGINE_BATCH];
    uint32_t k = 0, ne = 0;
    for (EngineReq *r = first; r && k < n; r = r->next) v[k++] = r;
    /* encrypt records first */
    std::stable_partition(v, v + n, [](const EngineReq *r) { return !r->dec; });
    while (ne < n && !v[ne]->dec) ne++;
    const size_t off_res = align_up((size_t) n * sizeof(tlsrec_batch_rec), 256);
    const size_t off_arena = align_up(off_res + (size_t) n * sizeof(tlsrec_batch_res), 256);
    size_t used = 0;
    size_t boff[ENGINE_BATCH];
    for (uint32_t i = 0; i < n; i++) {
        boff[i] = used;
        used = align_up(used + v[i]->buf_len + v[i]->d.cid_len + 16, ENGINE_ALIGN);
    }
    const size_t need = off_arena + used + ENGINE_ALIGN;
    bool fail_alloc = false;
#ifdef TLSREC_TEST_HOOKS
    if (g_test_fail_staging > 0) {
        g_test_fail_staging--;
        fail_alloc = true;
    }
#endif
    if (S.cap < need || fail_alloc) {
        hipStreamSynchronize(S.st);
        hipHostFree(S.h);
        hipFree(S.d);
        S.h = S.hd = S.d = NULL;
        S.cap = 0;
        const size_t want = need > (1u << 20) ? need + need / 2 : (1u << 20);
        if (fail_alloc || hipHostMalloc((void **) &S.h, want, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void **) &S.hd, S.h, 0) != hipSuccess ||
            hipMalloc((void **) &S.d, want) != hipSuccess) {
            /* no request of this batch ran: each caller gets the error, never
             * the unfilled result (ssl_msg.c:1260 / :1804) */
            if (S.h) hipHostFree(S.h);
            if (S.d) hipFree(S.d);
            S.h = S.hd = S.d = NULL;
            for (uint32_t i = 0; i < n; i++) v[i]->rc = TLSREC_ERR_SSL_ALLOC_FAILED;
            return TLSREC_ERR_SSL_ALLOC_FAILED;
        }
        S.cap = want;
    }
    tlsrec_batch_rec *hd = (tlsrec_batch_rec *) S.h;
    tlsrec_batch_res *hr = (tlsrec_batch_res *) (S.h + off_res);
    uint8_t *ha = S.h + off_arena;
    uint32_t mask_e = 0, mask_d = 0;
    for (uint32_t i = 0; i < n; i++) {
        EngineReq *r = v[i];
        tlsrec_batch_rec d = r->d;
        d.buf_off = boff[i];
        if (r->buf_len) memcpy(ha + boff[i], r->buf, r->buf_len);
        if (d.cid_len) {
            memcpy(ha + boff[i] + r->buf_len, r->cid, d.cid_len);
            const uint32_t o = (uint32_t) r->buf_len;
            d.cid_off[0] = (uint8_t) o; d.cid_off[1] = (uint8_t) (o >> 8);
            d.cid_off[2] = (uint8_t) (o >> 16); d.cid_off[3] = (uint8_t) (o >> 24);
        }
        hd[i] = d;
        /* each result goes up as INTERNAL_ERROR: only a kernel turns it into a
         * verdict (ssl_msg.c:1260 / :1804, auth_done) */
        memset(&hr[i], 0, sizeof(hr[i]));
        hr[i].status = TLSREC_ERR_SSL_INTERNAL_ERROR;
        (r->dec ? mask_d : mask_e) |= 1u << r->cipher;
    }
    const size_t total = off_arena + used;
    const bool zc = total <= engine_zc_max();
    uint8_t *base = zc ? S.hd : S.d;
    hipError_t e = zc ? hipSuccess : hipMemcpyAsync(S.d, S.h, total, hipMemcpyHostToDevice, S.st);
    int rc = e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    tlsrec_batch_rec *dd = (tlsrec_batch_rec *) base;
    tlsrec_batch_res *dr = (tlsrec_batch_res *) (base + off_res);
    uint8_t *da = base + off_arena;
    BatchOpt o;
    o.prefilled = true;
    o.coalesced = true;     /* identity order, a wave per GCM record (one record too: 8 KiB of tables, not 56) */
    if (!rc && ne) {
        o.only_mask = mask_e;
        rc = batch(kt, dd, dr, ne, da, da, 0, S.st, 0, o);
    }
    if (!rc && n > ne) {
        o.only_mask = mask_d;
        rc = batch(kt, dd + ne, dr + ne, n - ne, da, da, 0, S.st, 1, o);
    }
    if (!rc) {
        e = zc ? hipSuccess : hipMemcpyAsync(S.h + off_res, S.d + off_res, total - off_res, hipMemcpyDeviceToHost, S.st);
        if (e == hipSuccess) e = hipStreamSynchronize(S.st);
        if (e != hipSuccess) rc = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    } else {
        hipStreamSynchronize(S.st);
    }
    for (uint32_t i = 0; i < n; i++) {
        EngineReq *r = v[i];
        r->rc = rc;
        if (!rc) {
            r->res = hr[i];
            if (r->buf_len) memcpy(r->buf, ha + boff[i], r->buf_len);
        }
    }
    return rc;
}

/* Run one record through the kernels: host buffer -> device -> host.  A
 * decrypted record's CID (cid_len bytes) is staged right after the buffer.
 * AES-GCM and ChaCha20-Poly1305 records of transforms without connection IDs
 * go to the record server first (plan: the record's framing plan, as the
 * host entry points computed it); the coalescing launch path below takes
 * every other record, and any the server does not take. */
extern "C" int tlsrec__engine_run(int dec, const tlsrec_batch_rec *rec, unsigned char *buf, size_t buf_len,
                                  const unsigned char *cid, const void *plan, tlsrec_batch_res *out)
{
    if (!g_ready) {
        pthread_mutex_lock(&g_mu);
        int r = engine_init_locked();
        pthread_mutex_unlock(&g_mu);
        if (r) return r;
    }
    uint32_t idx = 0;
    tlsrec_keytab *kt = slot_table((int) rec->slot, &idx);
    if (!kt) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    const uint32_t cipher = (uint32_t) tlsrec__keytab_cipher(kt, idx);
    if (cipher == 0) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (buf_len > 0xffffffffu - 64) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* per slot, not the page's has_cid: one CID connection must not take the
     * server away from the page's other 4095 slots */
    if ((tlsrec_cipher_is_gcm((int) cipher) || cipher == TLSREC_CIPHER_CHACHA20_POLY1305) &&
        !g_pages[rec->slot / ENGINE_PAGE_SLOTS].cid[idx] && rec->cid_len == 0) {
        tlsrec_batch_rec d = *rec;
        d.slot = idx;
        const uint4 *tab = tlsrec__keytab_ghtab(kt) + (size_t) idx * KEY_TABLE_WORDS;
        const void *p_state = tlsrec__keytab_slots(kt) + idx, *p_ghtab = tab, *p_hpw = tab + KEY_HPOW_OFF;
#ifdef TLSREC_TEST_HOOKS
        if (g_test_shadow) {
            /* copies at the first address of the test's buffer whose low word
             * has bit 31 set, all three inside that half of the 4 GiB window */
            const size_t sz[3] = { sizeof(SlotState), sizeof(uint4) * KEY_TABLE_WORDS, 0 };
            const size_t tot = sz[0] + sz[1] + sz[2];
            const uintptr_t b0 = (uintptr_t) g_test_shadow, end = b0 + g_test_shadow_bytes;
            uintptr_t at = (b0 + 255) & ~(uintptr_t) 255;
            if (!(at & 0x80000000u) || (at & 0xffffffffu) + tot > 0x100000000ull)
                at = ((at & 0xffffffffu) + tot > 0x100000000ull ? (at | 0xffffffffull) + 1 : at & ~(uintptr_t) 0xffffffffu) |
                     0x80000000u;
            if (at + tot > end) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
            const void *src[3] = { p_state, p_ghtab, p_hpw };
            uint8_t *dst = (uint8_t *) at;
            const void *dsts[3];
            for (int k = 0; k < 3; k++) {
                if (hipMemcpyAsync(dst, src[k], sz[k], hipMemcpyDeviceToDevice, g_load) != hipSuccess)
                    return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
                dsts[k] = dst;
                dst += sz[k];
            }
            if (hipStreamSynchronize(g_load) != hipSuccess) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
            p_state = dsts[0];
            p_ghtab = dsts[1];
            p_hpw = (const uint4 *) dsts[1] + KEY_HPOW_OFF;    /* the powers inside the copied tables */
        }
#endif
        const int r = tlsrec__server_run(dec, cipher, tlsrec_cipher_nr((int) cipher), &d, p_state, p_ghtab, p_hpw,
                                         buf, buf_len, plan, tlsrec__test_skip() == 0, out);
        if (r <= 0) return r;
    }
    Combiner *co = g_pages[rec->slot / ENGINE_PAGE_SLOTS].co[engine_queue(cipher, dec)];
    EngineReq me;
    me.dec = dec;
    me.d = *rec;
    me.d.slot = idx;
    me.cipher = cipher;
    me.buf = buf;
    me.buf_len = buf_len;
    me.cid = cid;
    /* fail closed: a request no batch filled in reads as an error, never as
     * the success its zeroed result would say */
    me.rc = TLSREC_ERR_SSL_INTERNAL_ERROR;
    memset(&me.res, 0, sizeof(me.res));
    me.res.status = TLSREC_ERR_SSL_INTERNAL_ERROR;
    me.done = 0;
    me.next = NULL;
    pthread_mutex_lock(&co->mu);
    if (co->tail) co->tail->next = &me; else co->head = &me;
    co->tail = &me;
    while (!me.done) {
        int si = -1;
        for (int i = 0; i < ENGINE_SETS; i++)
            if (!co->set[i].busy) { si = i; break; }
        if (si < 0 || co->head == NULL) {
            pthread_cond_wait(&co->cv, &co->mu);
            continue;
        }
        /* leader: take the queue (up to ENGINE_BATCH records) */
        EngineSet &S = co->set[si];
        S.busy = 1;
        EngineReq *first = co->head;
        uint32_t n = 0;
        EngineReq *last = NULL;
        for (EngineReq *r = first; r && n < ENGINE_BATCH; r = r->next) { last = r; n++; }
        co->head = last->next;
        if (!co->head) co->tail = NULL;
        last->next = NULL;
        co->batches++;
        co->records += n;
        pthread_mutex_unlock(&co->mu);
        run_batch(kt, S, first, n);
        pthread_mutex_lock(&co->mu);
        for (EngineReq *r = first, *nx; r; r = nx) {
            nx = r->next;
            r->done = 1;
        }
        S.busy = 0;
        pthread_cond_broadcast(&co->cv);
    }
    pthread_mutex_unlock(&co->mu);
    if (me.rc) return me.rc;
    *out = me.res;
    return 0;
}

/* coalescing statistics: batches run and records carried by the queues [q0, q1) of every page */
static void sum_stats(int q0, int q1, uint64_t *batches, uint64_t *records)
{
    uint64_t b = 0, r = 0;
    for (int pg = 0; pg < g_npages; pg++)
        for (int q = q0; q < q1; q++) {
            Combiner *c = g_pages[pg].co[q];
            if (!c) continue;
            pthread_mutex_lock(&c->mu);
            b += c->batches;
            r += c->records;
            pthread_mutex_unlock(&c->mu);
        }
    if (batches) *batches = b;
    if (records) *records = r;
}

/* one queue (engine_queue: family * 2 + direction; families GCM, ChaCha20-Poly1305, CCM, CBC) */
extern "C" int tlsrec__engine_queue_stats(int queue, uint64_t *batches, uint64_t *records)
{
    if (queue < 0 || queue >= ENGINE_QUEUES) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    sum_stats(queue, queue + 1, batches, records);
    return 0;
}

extern "C" void tlsrec__engine_stats(uint64_t *batches, uint64_t *records)
{
    sum_stats(0, ENGINE_QUEUES, batches, records);
}
