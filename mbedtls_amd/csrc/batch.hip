/*
 * batch.hip -- one batch of records through the kernels: the bucket pass that groups records by key, the
 * launch of every cipher family the table holds (shaped by tlsrec_plan.h), and the tlsrec_batch_* entry
 * points.  The host pipeline (host_pipe.hip) and the single-record engine (engine.hip) run their batches
 * through batch() with options of their own (tlsrec_internal.h BatchOpt).
 *
 * Plain HIP runtime C++: no kernel here, a record is only ever transformed by the kernel units.
 */
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_frame.h"
#include "tlsrec_internal.h"
#include "tlsrec_keytab.h"
#include "tlsrec_plan.h"

using namespace tlsrec;

/* The launch shapes are decided in tlsrec_plan.h, host functions without a
 * device; exported (the release library too) so that they can be checked on a
 * CPU.  knobs == NULL: the TLSREC_GCM_* switches of the environment. */
static_assert(PLAN_GCM_WAVES == GCM_WAVES && PLAN_CP_WAVES == CP_WAVES, "tlsrec_plan.h workgroup shapes");

extern "C" uint32_t tlsrec__gcm_pair_small_l(uint32_t rpk) { return gcm_pair_small_l(rpk); }

extern "C" void tlsrec__gcm_plan(const GcmPlanIn *in, const GcmKnobs *knobs, GcmPlan *out)
{
    *out = gcm_plan(*in, knobs ? *knobs : gcm_knobs_from_env());
}

extern "C" void tlsrec__chacha_plan(uint32_t n, uint32_t cu, uint32_t lanes_in, int has_cid, ChachaPlan *out)
{
    *out = chacha_plan(n, cu, lanes_in, has_cid != 0);
}

/* Device scratch of one bucketed batch (the stream's kind-0 scratch). */
struct BucketScratch {
    tlsrec_scratch_lease lease = { nullptr, nullptr };
    uint32_t *counts, *offs, *perm;
    uint2 *keyrank;
    bool want_srecs = false;  /* GCM kernels will run: keep the descriptors in perm order too */
    tlsrec_batch_rec *srecs = nullptr;
    void *scan_tmp;           /* tlsrec__exclusive_scan's block sums */
    size_t scan_bytes;
};

/* The bucket pass's classes, in the order of its keys (BucketArgs): a class of
 * `capacity` keys per slot kind, except ChaCha20-Poly1305's CP_SPREAD counters. */
enum BucketClass {
    BC_AES_GCM = 0,       /* + 0 / 1 / 2: AES-128 / -256 / -192-GCM */
    BC_CCM = 3,
    BC_CHACHA = 4,
    BC_ALT_GCM = 5,       /* + 0 .. 5: ARIA-128/192/256-GCM, Camellia-128/192/256-GCM */
    BC_CBC = 11,          /* counted only while the table holds a CBC slot */
    BC_IDENTITY = -1      /* no class: the descriptors in their own order, whatever the batch's */
};

struct ClassRange {
    size_t lo, hi;        /* the class's keys [lo, hi): where its offsets start in BucketScratch::offs */
};

static ClassRange bucket_class_range(int cls, uint32_t capacity)
{
    const size_t cap = capacity;
    if (cls < BC_CHACHA) return { cls * cap, (cls + 1) * cap };
    if (cls == BC_CHACHA) return { 4 * cap, 4 * cap + CP_SPREAD };
    return { (cls - 1) * cap + CP_SPREAD, cls * cap + CP_SPREAD };
}

static int bucket(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res, uint32_t n,
                  hipStream_t st, BucketScratch &b)
{
    /* every class up to the last the table can hold, and the end */
    const size_t nk = bucket_class_range((kt->cipher_mask & CBC_CIPHER_BITS) ? BC_CBC : BC_CBC - 1, kt->capacity).hi + 1;
    b.scan_bytes = tlsrec__scan_scratch_bytes((uint32_t) nk);
    const size_t szk = align_up(nk * 4, 256), szp = align_up((size_t) n * 4, 256), szr = align_up((size_t) n * 8, 256);
    /* the descriptors in perm order for the GCM kernels (GcmArgs::srecs) */
    const size_t szs = b.want_srecs ? align_up((size_t) n * sizeof(tlsrec_batch_rec), 256) : 0;
    const size_t total = 2 * szk + szp + szr + szs + b.scan_bytes + 256;
    const int lr = tlsrec__scratch_acquire(st, 0, total, &b.lease);
    if (lr) return lr;
    uint8_t *m = (uint8_t *) b.lease.mem;
    b.counts = (uint32_t *) m;
    b.offs = (uint32_t *) (m + szk);
    b.perm = (uint32_t *) (m + 2 * szk);
    b.keyrank = (uint2 *) (m + 2 * szk + szp);
    b.srecs = szs ? (tlsrec_batch_rec *) (m + 2 * szk + szp + szr) : nullptr;
    b.scan_tmp = m + 2 * szk + szp + szr + szs;
    BucketArgs a;
    a.slots = kt->d_slots;
    a.cipher_of = kt->d_cipher;
    a.recs = recs;
    a.res = res;
    a.n = n;
    a.capacity = kt->capacity;
    a.counts = b.counts;
    a.offs = b.offs;
    a.keyrank = b.keyrank;
    a.nk = (uint32_t) nk;
    a.perm = b.perm;
    a.srecs = b.srecs;
    if (tlsrec__launch_bucket_zero(&a, st) != hipSuccess ||
        tlsrec__launch_bucket_count(&a, st) != hipSuccess ||
        tlsrec__exclusive_scan(b.counts, b.offs, (uint32_t) nk, (uint32_t *) b.scan_tmp, st) != hipSuccess ||
        tlsrec__launch_bucket_scatter(&a, st) != hipSuccess)
        return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    return 0;
}

/* Test hooks (tlsrec_internal.h TLSREC_HOOK_SKIP; the test build only, as the
 * reference compiles its own under MBEDTLS_TEST_HOOKS, ssl_misc.h:2685):
 *   tlsrec__test_skip_record   the AEAD kernels leave this record index
 *                              unreached, so a test can show that its result
 *                              stays INTERNAL_ERROR
 *   tlsrec__test_launch_log_*  the dispatchers' choices (tlsrec_internal.h
 *                              TLSREC_LAUNCH_LOG): the last LAUNCH_LOG_CAP
 *                              entries, oldest first
 * (the single-record engine's own hooks: engine.hip) */
#ifdef TLSREC_TEST_HOOKS
static volatile uint32_t g_test_skip = 0xffffffffu;

extern "C" void tlsrec__test_skip_record(uint32_t index) { g_test_skip = index; }

#define LAUNCH_LOG_CAP 256
static pthread_mutex_t g_launch_log_mu = PTHREAD_MUTEX_INITIALIZER;
static int32_t g_launch_log[LAUNCH_LOG_CAP][5];
static uint64_t g_launch_log_n = 0;      /* entries appended since the reset */

extern "C" void tlsrec__test_launch_log_add(int32_t kind, int32_t p0, int32_t p1, int32_t p2, int32_t p3)
{
    pthread_mutex_lock(&g_launch_log_mu);
    int32_t *e = g_launch_log[g_launch_log_n++ % LAUNCH_LOG_CAP];
    e[0] = kind;
    e[1] = p0;
    e[2] = p1;
    e[3] = p2;
    e[4] = p3;
    pthread_mutex_unlock(&g_launch_log_mu);
}
extern "C" void tlsrec__test_launch_log_reset(void)
{
    pthread_mutex_lock(&g_launch_log_mu);
    g_launch_log_n = 0;
    pthread_mutex_unlock(&g_launch_log_mu);
}
/* the last min(appended, LAUNCH_LOG_CAP, cap) entries, oldest first, as 5 x
 * int32 each; returns how many were written */
extern "C" uint32_t tlsrec__test_launch_log_read(int32_t *entries, uint32_t cap)
{
    pthread_mutex_lock(&g_launch_log_mu);
    uint64_t have = g_launch_log_n < LAUNCH_LOG_CAP ? g_launch_log_n : LAUNCH_LOG_CAP;
    if (have > cap) have = cap;
    for (uint64_t k = 0; k < have; k++)
        memcpy(entries + 5 * k, g_launch_log[(g_launch_log_n - have + k) % LAUNCH_LOG_CAP], sizeof(g_launch_log[0]));
    pthread_mutex_unlock(&g_launch_log_mu);
    return (uint32_t) have;
}
#else
static constexpr uint32_t g_test_skip = 0xffffffffu;
#endif
uint32_t tlsrec__test_skip(void) { return g_test_skip; }

/* Batch work takes the CUs the record server holds (server.hip): yield first,
 * note the batch's stream on every way out (the server launches no grid
 * between the two). */
struct YieldGuard {
    hipStream_t st;
    bool on;
    int counted;      /* the yield counted this batch as queueing (only then does the note uncount it) */
    YieldGuard(hipStream_t s, bool o) : st(s), on(o), counted(o ? tlsrec__server_yield() : 0) {}
    ~YieldGuard() { if (on) tlsrec__server_note_batch(st, counted); }
};

/* What every launch of one batch is given. */
struct BatchView {
    const tlsrec_keytab *kt;
    const tlsrec_batch_rec *recs;
    tlsrec_batch_res *res;
    uint32_t n;
    const uint8_t *in;
    uint8_t *out;
    hipStream_t st;
    int dec;
    uint32_t cmask;             /* 1 << TLSREC_CIPHER_* of the kernels to launch */
    uint32_t skip;              /* test hook (tlsrec__test_skip_record) */
    const BucketScratch *bs;    /* the bucket pass's order; nullptr = identity order */
};

static const uint32_t GCM_CIPHER_BITS =
    (1u << TLSREC_CIPHER_AES_128_GCM) | (1u << TLSREC_CIPHER_AES_256_GCM) | (1u << TLSREC_CIPHER_AES_192_GCM) |
    (1u << TLSREC_CIPHER_ARIA_128_GCM) | (1u << TLSREC_CIPHER_ARIA_192_GCM) | (1u << TLSREC_CIPHER_ARIA_256_GCM) |
    (1u << TLSREC_CIPHER_CAMELLIA_128_GCM) | (1u << TLSREC_CIPHER_CAMELLIA_192_GCM) |
    (1u << TLSREC_CIPHER_CAMELLIA_256_GCM);

/* The fields GcmArgs, CpArgs, CcmArgs and CbcArgs share, for the records of
 * bucket class cls; every other field zero or its default. */
template <class A> static A class_args(const BatchView &v, int cls)
{
    A a = A();
    a.slots = v.kt->d_slots;
    a.recs = v.recs;
    a.res = v.res;
    a.n = v.n;
    if (v.bs && cls != BC_IDENTITY) {
        const ClassRange r = bucket_class_range(cls, v.kt->capacity);
        a.perm = v.bs->perm;
        a.lo = v.bs->offs + r.lo;
        a.hi = v.bs->offs + r.hi;
    }
    a.in = v.in;
    a.out = v.out;
    a.capacity = v.kt->capacity;
    a.skip = v.skip;
    return a;
}

static GcmArgs gcm_args(const BatchView &v, int cls, int cipher)
{
    GcmArgs a = class_args<GcmArgs>(v, cls);
    a.ghtab = v.kt->d_ghtab;
    a.dummy = v.kt->d_dummy;
    a.srecs = v.bs ? v.bs->srecs : nullptr;
    a.cipher = (uint32_t) cipher;
    return a;
}

/* A table holding a single key, or a batch of one record, needs no grouping:
 * the kernels walk the descriptors in order and flag records naming an
 * unusable slot.  Neither does (r05) a table of ChaCha20-Poly1305 keys only:
 * its kernel walks records in arrival order, with or without the bucket
 * pass's permutation (the count / scan / scatter kernels cost 5-6 % of a
 * 1 M-record stream or DTLS batch), nor do (r06) records already grouped by
 * key -- the stream and DTLS layers emit each connection's records together,
 * and the GCM passes find a key's run of records where they lie (~90 us of a
 * 1 M-record call).  Otherwise the bucket pass groups the records by key.
 * Either way every result reads INTERNAL_ERROR before the AEAD kernels run
 * (the guard kernel, or the bucket count kernel), so a record that no kernel
 * reaches fails closed -- the reference's auth_done check, ssl_msg.c:1260 /
 * :1804. */
static int order_records(BatchView &v, const BatchOpt &opt, const GcmKnobs &knobs, bool identity, BucketScratch &bs)
{
    TLSREC_LAUNCH_LOG(TLSREC_LOG_BUCKET, !identity, 0, 0, 0);
    if (identity)
        return opt.prefilled ? 0 : hip_ok(tlsrec__launch_res_guard(v.res, v.n, v.st));
    bs.want_srecs = (v.cmask & GCM_CIPHER_BITS) != 0 && knobs.srecs;
    const int r = bucket(v.kt, v.recs, v.res, v.n, v.st, bs);
    if (!r) v.bs = &bs;
    return r;
}

/* AES-GCM: one launch per key size the table holds, shaped by gcm_plan() */
static int launch_aes_gcm(const BatchView &v, const BatchOpt &opt, const GcmKnobs &knobs, uint32_t lanes, bool keyrun)
{
    static const int ciphers[3] = { TLSREC_CIPHER_AES_128_GCM, TLSREC_CIPHER_AES_256_GCM, TLSREC_CIPHER_AES_192_GCM };
    GcmPlanIn in;
    in.n = v.n;
    in.nloaded = v.kt->nloaded;     /* read once: the engine's pages change under it */
    in.cu = (uint32_t) v.kt->cu;
    in.avg_bytes = opt.avg_bytes;
    in.lanes = lanes ? lanes : knobs.lanes;
    in.has_cid = v.kt->has_cid;
    in.coalesced = opt.coalesced;
    in.keyrun = keyrun;
    for (int ci = 0; ci < 3; ci++) {
        if (!(v.cmask & (1u << ciphers[ci]))) continue;
        in.nr = tlsrec_cipher_nr(ciphers[ci]);
        const GcmPlan p = gcm_plan(in, knobs);
        GcmArgs a = gcm_args(v, BC_AES_GCM + ci, ciphers[ci]);
        a.rpw = p.rpw;
        a.g5 = p.g5;
        a.tm = p.tm;
        a.src_off = v.dec ? nullptr : opt.src_off;
        TLSREC_LAUNCH_LOG(TLSREC_LOG_GCM, p.L, p.code, a.tm, a.src_off != nullptr);
        if (tlsrec__launch_gcm(&a, v.dec, p.L, (int) in.nr, p.code, p.grid, v.st) != hipSuccess)
            return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    return 0;
}

/* ARIA-GCM and Camellia-GCM: the GCM kernel around the LDS-table cipher, one
 * configuration (8 lanes, 16 waves) */
static int launch_alt_gcm(const BatchView &v)
{
    static const int ciphers[6] = { TLSREC_CIPHER_ARIA_128_GCM, TLSREC_CIPHER_ARIA_192_GCM,
                                    TLSREC_CIPHER_ARIA_256_GCM, TLSREC_CIPHER_CAMELLIA_128_GCM,
                                    TLSREC_CIPHER_CAMELLIA_192_GCM, TLSREC_CIPHER_CAMELLIA_256_GCM };
    for (int ci = 0; ci < 6; ci++) {
        const int c = ciphers[ci];
        if (!(v.cmask & (1u << c))) continue;
        GcmArgs a = gcm_args(v, BC_ALT_GCM + ci, c);
        a.rpw = pick_rpw(v.n, (uint32_t) ARIA_GCM_WAVES, 8u, (uint32_t) v.kt->cu);
        const uint32_t grid = plan_grid(v.n, (uint32_t) ARIA_GCM_WAVES, a.rpw);
        TLSREC_LAUNCH_LOG(TLSREC_LOG_ALT_GCM, c, 0, 0, 0);
        if (tlsrec__launch_gcm_aria(&a, v.dec, (int) tlsrec_cipher_alt_nr(c), (int) v.kt->has_cid, grid, v.st) !=
            hipSuccess)
            return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    return 0;
}

/* CCM, every block cipher: one launch, the rounds the table holds as a mask */
static int launch_ccm(const BatchView &v)
{
    uint32_t ccm_nr = 0;
    for (int c = TLSREC_CIPHER_AES_128_CCM; c <= TLSREC_CIPHER_AES_256_CCM_8; c++)
        if (v.cmask & (1u << c)) ccm_nr |= 1u << tlsrec_cipher_nr(c);
    for (int c = TLSREC_CIPHER_ARIA_128_CCM; c <= TLSREC_CIPHER_CAMELLIA_256_CCM; c++)   /* ARIA / Camellia: bit nr + 4 */
        if (tlsrec_cipher_is_alt_ccm(c) && (v.cmask & (1u << c))) ccm_nr |= 1u << (tlsrec_cipher_alt_nr(c) + 4);
    if (!ccm_nr) return 0;
    CcmArgs a = class_args<CcmArgs>(v, BC_CCM);
    a.cid = v.kt->has_cid;
    TLSREC_LAUNCH_LOG(TLSREC_LOG_CCM, ccm_nr, 0, 0, 0);
    return hip_ok(tlsrec__launch_ccm(&a, v.dec, ccm_nr, v.st));
}

/* CBC + HMAC: one launch per (cipher, MAC) the table holds.  The coalesced single-record path decrypts
 * with a wave per record (cbc_wave.hip; TLSREC_CBC_WAVE=0: the lane kernel there too); encryption, two
 * dependent chains, and every other batch stay on the lane kernel. */
static int launch_cbc(const BatchView &v, const BatchOpt &opt, bool wave_knob)
{
    if (!(v.cmask & CBC_CIPHER_BITS)) return 0;
    uint32_t variants = v.kt->cbc_variants, macs = 0;
    for (int c = TLSREC_CIPHER_CBC_FIRST; c <= TLSREC_CIPHER_CBC_LAST; c++) {
        const uint32_t three = 7u << (3 * (c - TLSREC_CIPHER_CBC_FIRST));     /* the cipher's MACs */
        if (!(v.cmask & (1u << c))) variants &= ~three;
        macs |= (variants & three) >> (3 * (c - TLSREC_CIPHER_CBC_FIRST));
    }
    CbcArgs a = class_args<CbcArgs>(v, BC_CBC);
    a.ghtab = v.kt->d_ghtab;
    /* (p3: the ARIA / Camellia variants, from the bit of ARIA-128 with MAC 1 up; AES alone logs what it always has) */
    TLSREC_LAUNCH_LOG(TLSREC_LOG_CBC, v.dec, macs << 1, v.kt->cbc_etm,
                      variants >> (3 * (TLSREC_CIPHER_ARIA_128_CBC - TLSREC_CIPHER_CBC_FIRST)));
    const bool wave = opt.coalesced && v.dec && wave_knob;
    TLSREC_LAUNCH_LOG(TLSREC_LOG_CBC_KERNEL, wave, v.dec, 0, 0);
    if (wave) return hip_ok(tlsrec__launch_cbc_wave(&a, variants, v.st));
    return hip_ok(tlsrec__launch_cbc(&a, v.dec, variants, v.st));
}

/* ChaCha20-Poly1305, shaped by chacha_plan(); lanes_in: the caller's own request */
static int launch_chacha(const BatchView &v, const BatchOpt &opt, uint32_t lanes_in)
{
    if (!(v.cmask & (1u << TLSREC_CIPHER_CHACHA20_POLY1305))) return 0;
    const ChachaPlan p = chacha_plan(v.n, (uint32_t) v.kt->cu, lanes_in, v.kt->has_cid != 0);
    CpArgs a = class_args<CpArgs>(v, BC_CHACHA);
    a.rpw = p.rpw;
    a.cid = v.kt->has_cid;
    a.src_off = v.dec ? nullptr : opt.src_off;
    TLSREC_LAUNCH_LOG(TLSREC_LOG_CHACHA, p.L, a.src_off != nullptr, 0, 0);
    return hip_ok(tlsrec__launch_chachapoly(&a, v.dec, p.L, p.grid, v.st));
}

/* BatchOpt::no_cbc over a table with CBC slots: their records get the bad-slot result */
static int launch_cbc_refusal(const BatchView &v, const BatchOpt &opt)
{
    if (!opt.no_cbc || !(v.kt->cipher_mask & CBC_CIPHER_BITS)) return 0;
    CbcArgs a = class_args<CbcArgs>(v, BC_IDENTITY);
    a.ghtab = v.kt->d_ghtab;
    return hip_ok(tlsrec__launch_cbc_refuse(&a, v.st));
}

int tlsrec::batch(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res, uint32_t n,
                  const uint8_t *in, uint8_t *out, uint32_t lanes, void *stream, int dec, const BatchOpt &opt)
{
    if (!kt || (!recs && n) || (!res && n)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    YieldGuard yg(st, !opt.coalesced);
    const GcmKnobs knobs = gcm_knobs_from_env();
    const bool cbc_wave = plan_env("TLSREC_CBC_WAVE", 1) != 0;
    const uint32_t cmask = (opt.only_mask ? (kt->cipher_mask & opt.only_mask) : kt->cipher_mask) &
                           (opt.no_cbc ? ~CBC_CIPHER_BITS : ~0u);
    BatchView v = { kt, recs, res, n, in, out, st, dec, cmask, g_test_skip, nullptr };
    const bool grouped = opt.grouped && knobs.grouped;
    const bool identity = kt->nloaded == 1 || n == 1 || opt.coalesced || grouped ||
                          kt->cipher_mask == (1u << TLSREC_CIPHER_CHACHA20_POLY1305);
    const bool keyrun = !identity || grouped;     /* the many-keys launch shapes apply */
    BucketScratch bs;
    int rc = order_records(v, opt, knobs, identity, bs);
    if (!rc) rc = launch_aes_gcm(v, opt, knobs, lanes, keyrun);
    if (!rc) rc = launch_alt_gcm(v);
    if (!rc) rc = launch_ccm(v);
    if (!rc) rc = launch_cbc(v, opt, cbc_wave);
    if (!rc) rc = launch_chacha(v, opt, lanes);
    if (!rc) rc = launch_cbc_refusal(v, opt);
    tlsrec__scratch_release(&bs.lease);
    return rc;
}


extern "C" int tlsrec_batch_encrypt(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                                    uint32_t n, const uint8_t *in_arena, uint8_t *out_arena,
                                    uint32_t lanes_per_record, void *stream)
{
    return batch(kt, recs, res, n, in_arena, out_arena, lanes_per_record, stream, 0);
}

extern "C" int tlsrec_batch_decrypt(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                                    uint32_t n, const uint8_t *in_arena, uint8_t *out_arena,
                                    uint32_t lanes_per_record, void *stream)
{
    return batch(kt, recs, res, n, in_arena, out_arena, lanes_per_record, stream, 1);
}

extern "C" int tlsrec_batch_encrypt_sized(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                                          uint32_t n, const uint8_t *in_arena, uint8_t *out_arena,
                                          uint32_t mean_record_bytes, void *stream)
{
    BatchOpt o;
    o.avg_bytes = mean_record_bytes;
    return batch(kt, recs, res, n, in_arena, out_arena, 0, stream, 0, o);
}

extern "C" int tlsrec_batch_decrypt_sized(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                                          uint32_t n, const uint8_t *in_arena, uint8_t *out_arena,
                                          uint32_t mean_record_bytes, void *stream)
{
    BatchOpt o;
    o.avg_bytes = mean_record_bytes;
    return batch(kt, recs, res, n, in_arena, out_arena, 0, stream, 1, o);
}

extern "C" int tlsrec__keytab_src_ok(const tlsrec_keytab *kt)
{
    const uint32_t ok = (1u << TLSREC_CIPHER_AES_128_GCM) | (1u << TLSREC_CIPHER_AES_192_GCM) |
                        (1u << TLSREC_CIPHER_AES_256_GCM) | (1u << TLSREC_CIPHER_CHACHA20_POLY1305);
    return kt && !kt->has_cid && (kt->cipher_mask & ~ok) == 0;   /* (the CID kernel variants read in place) */
}

extern "C" int tlsrec__keytab_has_cbc(const tlsrec_keytab *kt)
{
    return kt && (kt->cipher_mask & CBC_CIPHER_BITS) != 0;
}

extern "C" int tlsrec__batch_src(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                                 uint32_t n, const uint8_t *in_arena, uint8_t *out_arena, void *stream,
                                 uint32_t avg_bytes, const uint64_t *src_off)
{
    if (!tlsrec__keytab_src_ok(kt) || !src_off) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    BatchOpt o;
    o.avg_bytes = avg_bytes;
    o.src_off = src_off;
    o.grouped = true;                    /* (the stream / DTLS send paths' records, connection by connection) */
    o.no_cbc = true;
    return batch(kt, recs, res, n, in_arena, out_arena, 0, stream, 0, o);
}

extern "C" int tlsrec__batch_sized(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res,
                                   uint32_t n, const uint8_t *in_arena, uint8_t *out_arena, void *stream, int dec,
                                   uint32_t avg_bytes, int prefilled, int cbc)
{
    BatchOpt o;
    o.avg_bytes = avg_bytes;
    o.grouped = true;                    /* (the stream / DTLS layers' records, connection by connection) */
    o.no_cbc = cbc == 0;                 /* (cbc: the _ex calls with TLSREC_FRAME_CBC) */
    o.prefilled = prefilled != 0;
    return batch(kt, recs, res, n, in_arena, out_arena, 0, stream, dec, o);
}
