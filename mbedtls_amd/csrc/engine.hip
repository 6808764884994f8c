/*
 * engine.hip -- host side of the device engine: key tables, batch launches,
 * and the staging used by the single-record entry points.
 *
 * Everything here is plain HIP runtime C++ behind the extern "C" ABI of
 * include/tlsrec.h.  No torch types, no CPU crypto: a record is only ever
 * transformed by the kernels in kernels.hip.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_cbc.h"
#include "tlsrec_frame.h"
#include "tlsrec_internal.h"
#include "tlsrec_plan.h"

using namespace tlsrec;

struct HostPipe;   /* tlsrec_host_batch_*: device slots and streams, made on first use */

struct tlsrec_keytab {
    uint32_t capacity;
    int device;
    int cu;                   /* compute units of the device (launch sizing), read once at create */
    SlotState *d_slots;
    uint4 *d_ghtab;
    uint8_t *d_cipher;        /* each slot's cipher, one byte (the bucket pass reads it per record:
                                 an L2-resident array instead of a line of the 1 KiB slot) */
    tlsrec_key_material *d_stage;
    tlsrec_cbc_key_material *d_stage_cbc;   /* capacity records, made by the first CBC batch derivation */
    uint8_t *h_cipher;        /* host mirror of each slot's cipher */
    uint32_t cipher_mask;     /* 1 << TLSREC_CIPHER_* of every loaded slot */
    uint32_t nloaded;         /* slots holding a key */
    uint32_t cbc_variants;    /* CBC slots loaded: bit 3 * (cipher - CBC_FIRST) + (mac - 1) (tlsrec__launch_cbc) */
    uint32_t cbc_etm;         /* ... and bit etm: the MAC orders among them (launch log) */
    volatile uint32_t has_cid; /* some slot was given a DTLS connection ID: launch the CID kernels */
    uint8_t *d_dummy;         /* GcmArgs::dummy: 64 KiB the idle lanes of a wave-pass round load and store */
    HostPipe *pipe;
    pthread_mutex_t pipe_mu;
};

static int hip_ok(hipError_t e) { return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED; }

extern "C" int tlsrec_device_check(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    return 0;
}

extern "C" const char *tlsrec_version_string(void)
{
    return "tlsrec 0.2 gfx950: aes-128/192/256-gcm(L=4/8/16/64, T-tables in LDS, GHASH 4-bit position tables) "
           "aes-ccm/ccm_8(lane per record) chacha20-poly1305(L=1/2/4/8, 26-bit limbs) "
           "tls13-key-schedule(hkdf-sha256/384) stream-record-layer aria-128/192/256-gcm/ccm camellia-128/192/256-gcm/ccm dtls1.2-cid dtls1.2-datagram-record-layer(anti-replay) session-tickets aes-128/256-cbc-hmac-sha1/sha256/sha384(mac-then-encrypt, encrypt-then-mac; lane per record) aria-128/camellia-128-cbc-hmac-sha256 aria-256/camellia-256-cbc-hmac-sha384 cbc-hmac-single-record(decrypt: wave per record)";
}

extern "C" int tlsrec_keytab_create(tlsrec_keytab **out, uint32_t capacity)
{
    if (out == NULL || capacity == 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    *out = NULL;
    if (tlsrec_device_check() != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    tlsrec_keytab *kt = (tlsrec_keytab *) calloc(1, sizeof(*kt));
    if (!kt) return TLSREC_ERR_SSL_ALLOC_FAILED;
    kt->capacity = capacity;
    hipGetDevice(&kt->device);
    kt->cu = 256;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, kt->device) == hipSuccess && prop.multiProcessorCount > 0)
            kt->cu = prop.multiProcessorCount;
    }
    pthread_mutex_init(&kt->pipe_mu, NULL);
    kt->h_cipher = (uint8_t *) calloc(capacity, 1);
    if (!kt->h_cipher ||
        hipMalloc((void **) &kt->d_slots, sizeof(SlotState) * (size_t) capacity) != hipSuccess ||
        hipMalloc((void **) &kt->d_ghtab, sizeof(uint4) * (size_t) KEY_TABLE_WORDS * capacity) != hipSuccess ||
        hipMalloc((void **) &kt->d_cipher, (size_t) capacity) != hipSuccess ||
        hipMalloc((void **) &kt->d_stage, sizeof(tlsrec_key_material) * (size_t) capacity) != hipSuccess ||
        hipMalloc((void **) &kt->d_dummy, GCM_DUMMY_BYTES) != hipSuccess) {
        tlsrec_keytab_free(kt);
        return TLSREC_ERR_SSL_ALLOC_FAILED;
    }
    if (hipMemset(kt->d_slots, 0, sizeof(SlotState) * (size_t) capacity) != hipSuccess ||
        hipMemset(kt->d_cipher, 0, (size_t) capacity) != hipSuccess) {
        tlsrec_keytab_free(kt);
        return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    *out = kt;
    return 0;
}

extern "C" uint32_t tlsrec_keytab_capacity(const tlsrec_keytab *kt) { return kt ? kt->capacity : 0; }

/* host mirror of a slot's cipher (0 = never loaded) */
extern "C" int tlsrec__keytab_cipher(const tlsrec_keytab *kt, uint32_t slot)
{
    return kt && slot < kt->capacity ? kt->h_cipher[slot] : 0;
}

extern "C" int tlsrec_keytab_set_cid(tlsrec_keytab *kt, uint32_t slot, const unsigned char *cid, size_t cid_len,
                                     void *stream)
{
    if (kt == NULL || slot >= kt->capacity || cid_len > TLSREC_CID_LEN_MAX || (cid_len && cid == NULL))
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    uint8_t v[1 + TLSREC_CID_LEN_MAX];
    memset(v, 0, sizeof(v));
    v[0] = (uint8_t) cid_len;
    if (cid_len) memcpy(v + 1, cid, cid_len);
    if (cid_len) kt->has_cid = 1;
    static_assert(offsetof(SlotState, cid) == offsetof(SlotState, cid_len) + 1, "SlotState CID layout");
    hipStream_t st = (hipStream_t) stream;
    hipError_t e = hipMemcpyAsync(&kt->d_slots[slot].cid_len, v, sizeof(v), hipMemcpyHostToDevice, st);
    /* and its mirror in the slot's key material, which the kernels hold */
    if (e == hipSuccess) e = hipMemcpyAsync(&kt->d_slots[slot].km.reserved[0], v, 1, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

static void host_pipe_free(HostPipe *p);

extern "C" void tlsrec_keytab_free(tlsrec_keytab *kt)
{
    if (!kt) return;
    host_pipe_free(kt->pipe);
    pthread_mutex_destroy(&kt->pipe_mu);
    if (kt->d_slots) {
        /* zeroize key material (ssl_msg.c:6084-6099 zeroizes transforms) */
        hipMemset(kt->d_slots, 0, sizeof(SlotState) * (size_t) kt->capacity);
        hipMemset(kt->d_ghtab, 0, sizeof(uint4) * (size_t) KEY_TABLE_WORDS * kt->capacity);
        if (kt->d_dummy) hipMemset(kt->d_dummy, 0, GCM_DUMMY_BYTES);   /* idle lanes' keystream under the keys */
        if (kt->d_stage_cbc) hipMemset(kt->d_stage_cbc, 0, sizeof(tlsrec_cbc_key_material) * (size_t) kt->capacity);
        hipDeviceSynchronize();
    }
    hipFree(kt->d_dummy);
    hipFree(kt->d_slots);
    hipFree(kt->d_ghtab);
    hipFree(kt->d_cipher);
    hipFree(kt->d_stage);
    hipFree(kt->d_stage_cbc);
    free(kt->h_cipher);
    free(kt);
}

/* the ids cbc_is_cipher() accepts */
static const uint32_t CBC_CIPHER_BITS = (1u << TLSREC_CIPHER_AES_128_CBC) | (1u << TLSREC_CIPHER_AES_256_CBC) |
                                        (1u << TLSREC_CIPHER_ARIA_128_CBC) | (1u << TLSREC_CIPHER_ARIA_256_CBC) |
                                        (1u << TLSREC_CIPHER_CAMELLIA_128_CBC) |
                                        (1u << TLSREC_CIPHER_CAMELLIA_256_CBC);
static_assert(TLSREC_CIPHER_CBC_LAST < 32 && 3 * (TLSREC_CIPHER_CBC_LAST - TLSREC_CIPHER_CBC_FIRST) + 2 < 32,
              "cipher_mask and cbc_variants are 32-bit words");
/* Key setup of `count` checked CBC records (hk: their host copy, dk: the device copy the kernels read): one
 * launch per run of records of one kind (AES / ARIA or Camellia), so neither kernel meets the other's material */
static int launch_cbc_keysetup_runs(tlsrec_keytab *kt, const tlsrec_cbc_key_material *hk,
                                    const tlsrec_cbc_key_material *dk, uint32_t first, uint32_t count, hipStream_t st)
{
    for (uint32_t i = 0; i < count;) {
        const int alt = cbc_is_alt(hk[i].cipher);
        uint32_t j = i + 1;
        while (j < count && cbc_is_alt(hk[j].cipher) == alt) j++;
        const int r = hip_ok(tlsrec__launch_cbc_keysetup(kt->d_slots, kt->d_ghtab, kt->d_cipher, dk + i, first + i,
                                                         j - i, alt, st));
        if (r) return r;
        i = j;
    }
    return 0;
}

/* A slot that held a CBC key and now gets an AEAD one: its round keys of both
 * directions (SlotState::rk / rkr and ark, whichever way its cipher lays them
 * out) and HMAC midstates (the head of its table area) are not all
 * overwritten by the AEAD key setup, so one kernel zeroizes them,
 * enqueued before the key setup (a table that never held a CBC key: nothing). */
static int wipe_cbc_state(tlsrec_keytab *kt, uint32_t first, uint32_t count, hipStream_t st)
{
    if (!(kt->cipher_mask & CBC_CIPHER_BITS)) return 0;
    return hip_ok(tlsrec__launch_cbc_wipe(kt->d_slots, kt->d_ghtab, kt->d_cipher, first, count, st));
}

static int check_material(const tlsrec_key_material *k)
{
    if (k->cipher < TLSREC_CIPHER_AES_128_GCM || k->cipher > TLSREC_CIPHER_MAX)
        return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (k->tls_minor != 3 && k->tls_minor != 4) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (k->taglen != tlsrec_cipher_taglen(k->cipher)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (k->fixed_ivlen != 12 && k->fixed_ivlen != 4) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return 0;
}

extern "C" int tlsrec_keytab_load(tlsrec_keytab *kt, uint32_t first, uint32_t count,
                                  const tlsrec_key_material *keys, int keys_on_device, void *stream)
{
    if (!kt || !keys || first > kt->capacity || count > kt->capacity - first) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    tlsrec_key_material *host = NULL;
    if (keys_on_device) {
        host = (tlsrec_key_material *) malloc(sizeof(*host) * count);
        if (!host) return TLSREC_ERR_SSL_ALLOC_FAILED;
        if (hipMemcpyAsync(host, keys, sizeof(*host) * count, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            free(host);
            return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
        }
    }
    const tlsrec_key_material *hk = keys_on_device ? host : keys;
    for (uint32_t i = 0; i < count; i++) {
        int r = check_material(&hk[i]);
        if (r) {
            free(host);
            return r;
        }
    }
    if (wipe_cbc_state(kt, first, count, st)) {
        free(host);
        return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    for (uint32_t i = 0; i < count; i++) {
        if (kt->h_cipher[first + i] == 0) kt->nloaded++;
        kt->h_cipher[first + i] = hk[i].cipher;
        kt->cipher_mask |= 1u << hk[i].cipher;
    }
    free(host);
    const tlsrec_key_material *src = keys;
    if (!keys_on_device) {
        if (hipMemcpyAsync(kt->d_stage + first, keys, sizeof(*keys) * count, hipMemcpyHostToDevice, st) != hipSuccess)
            return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
        /* the staging copy must land before the host buffer may be reused */
        if (hipStreamSynchronize(st) != hipSuccess) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
        src = kt->d_stage + first;
    }
    return hip_ok(tlsrec__launch_keysetup(kt->d_slots, kt->d_ghtab, kt->d_cipher, src, first, count, st));
}

static int check_cbc_material(const tlsrec_cbc_key_material *k)
{
    /* unknown cipher or MAC, or an ARIA / Camellia id with a MAC no suite pairs it with */
    if (!cbc_pair_ok(k->cipher, k->mac)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (k->tls_minor != 3 || k->etm > 1) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return 0;
}

extern "C" int tlsrec_keytab_load_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count,
                                      const tlsrec_cbc_key_material *keys, int keys_on_device, void *stream)
{
    /* host material is judged first: its errors need neither a table nor a device */
    if (keys && !keys_on_device)
        for (uint32_t i = 0; i < count; i++) {
            const int r = check_cbc_material(&keys[i]);
            if (r) return r;
        }
    if (!kt || !keys || first > kt->capacity || count > kt->capacity - first) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    const size_t bytes = sizeof(*keys) * (size_t) count;
    /* the checks read the material on the host; device-resident material is
     * fetched for them, host material is staged on the device for the kernel */
    tlsrec_cbc_key_material *host = NULL, *dev = NULL;
    if (keys_on_device) {
        host = (tlsrec_cbc_key_material *) malloc(bytes);
        if (!host) return TLSREC_ERR_SSL_ALLOC_FAILED;
        if (hipMemcpyAsync(host, keys, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            free(host);
            return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
        }
    }
    const tlsrec_cbc_key_material *hk = keys_on_device ? host : keys;
    int r = 0;
    uint32_t variants = 0, etm = 0;
    for (uint32_t i = 0; i < count && !r; i++) {
        r = check_cbc_material(&hk[i]);
        if (!r) {
            variants |= cbc_variant_bit(hk[i].cipher, hk[i].mac);
            etm |= 1u << hk[i].etm;
        }
    }
    if (!r && !keys_on_device) {
        if (hipMalloc((void **) &dev, bytes) != hipSuccess) r = TLSREC_ERR_SSL_ALLOC_FAILED;
        else if (hipMemcpyAsync(dev, keys, bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
                 hipStreamSynchronize(st) != hipSuccess)
            r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    }
    if (!r) {
        for (uint32_t i = 0; i < count; i++) {
            if (kt->h_cipher[first + i] == 0) kt->nloaded++;
            kt->h_cipher[first + i] = hk[i].cipher;
            kt->cipher_mask |= 1u << hk[i].cipher;
        }
        kt->cbc_variants |= variants;
        kt->cbc_etm |= etm;
        r = launch_cbc_keysetup_runs(kt, hk, dev ? dev : keys, first, count, st);
    }
    if (host) {
        memset(host, 0, bytes);
        free(host);
    }
    if (dev) {
        /* the staged copy holds raw keys: wait for the kernel, zeroize, free */
        hipStreamSynchronize(st);
        hipMemset(dev, 0, bytes);
        hipFree(dev);
    }
    return r;
}

extern "C" uint32_t tlsrec_cbc_record_len(int mac, int etm, uint32_t content_len)
{
    return cbc_record_len(mac, etm, content_len);
}

/* what tlsrec_keytab_load_cbc accepts, for the host C of tlsrec_transform_setup_cbc: the key length of an
 * accepted (cipher, mac) pair, 0 for every other */
extern "C" uint32_t tlsrec__cbc_pair_keylen(int cipher, int mac)
{
    return cbc_pair_ok(cipher, mac) ? cbc_keylen(cipher) : 0u;
}

extern "C" uint32_t tlsrec__cbc_maclen(int mac) { return cbc_maclen(mac); }

extern "C" uint32_t tlsrec_cbc_minlen(int mac, int etm)
{
    const uint32_t ml = cbc_maclen(mac);
    if (ml == 0 || etm < 0 || etm > 1) return 0;
    /* ssl_tls.c:7822-7835: one block plus MAC, or the first multiple of the
     * block length above maclen; plus the explicit IV */
    return (etm ? ml + 16 : ml + 16 - ml % 16) + 16;
}

/* Device-side producers of key material (keysched.hip, tls13_ladder.hip, tls12_batch.hip) write into the
 * table's staging area and then commit: bookkeeping as tlsrec_keytab_load,
 * then the key-setup kernel on the staged slots. */
extern "C" tlsrec_key_material *tlsrec__keytab_stage(tlsrec_keytab *kt) { return kt->d_stage; }
extern "C" const SlotState *tlsrec__keytab_slots(const tlsrec_keytab *kt) { return kt->d_slots; }
extern "C" const uint4 *tlsrec__keytab_ghtab(const tlsrec_keytab *kt) { return kt->d_ghtab; }

extern "C" int tlsrec__keytab_commit_staged(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                            hipStream_t st)
{
    if (wipe_cbc_state(kt, first, count, st)) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    for (uint32_t i = 0; i < count; i++) {
        if (kt->h_cipher[first + i] == 0) kt->nloaded++;
        kt->h_cipher[first + i] = (uint8_t) cipher;
    }
    kt->cipher_mask |= 1u << cipher;
    return hip_ok(tlsrec__launch_keysetup(kt->d_slots, kt->d_ghtab, kt->d_cipher, kt->d_stage + first, first, count, st));
}

/* The same for CBC + HMAC material (tlsrec_tls12_keytab_derive_cbc): 128-byte
 * records, so a staging area of their own, allocated by the first call that
 * needs it (a table of AEAD slots only never pays for it); NULL = no memory. */
extern "C" tlsrec_cbc_key_material *tlsrec__keytab_stage_cbc(tlsrec_keytab *kt)
{
    if (!kt->d_stage_cbc &&
        hipMalloc((void **) &kt->d_stage_cbc, sizeof(tlsrec_cbc_key_material) * (size_t) kt->capacity) != hipSuccess)
        kt->d_stage_cbc = NULL;
    return kt->d_stage_cbc;
}

/* What tlsrec_keytab_load_cbc does after its checks, for `count` staged
 * records of one (cipher, mac, etm); then the staged range, which holds raw
 * MAC keys, is zeroized behind the key setup on the same stream (no wait). */
extern "C" int tlsrec__keytab_commit_staged_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, int mac,
                                                int etm, hipStream_t st)
{
    if (!kt->d_stage_cbc) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    for (uint32_t i = 0; i < count; i++) {
        if (kt->h_cipher[first + i] == 0) kt->nloaded++;
        kt->h_cipher[first + i] = (uint8_t) cipher;
    }
    kt->cipher_mask |= 1u << cipher;
    kt->cbc_variants |= cbc_variant_bit(cipher, mac);
    kt->cbc_etm |= 1u << etm;
    tlsrec_cbc_key_material *src = kt->d_stage_cbc + first;
    int r = hip_ok(tlsrec__launch_cbc_keysetup(kt->d_slots, kt->d_ghtab, kt->d_cipher, src, first, count,
                                               cbc_is_alt(cipher), st));
    if (hipMemsetAsync(src, 0, sizeof(*src) * (size_t) count, st) != hipSuccess && r == 0)
        r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    return r;
}

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

/* ---- per-stream device scratch (tlsrec_internal.h) ---- */
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

/* with g_scratch_mu held */
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
    const size_t al = 256;
    const size_t szk = (nk * 4 + al - 1) / al * al, szp = ((size_t) n * 4 + al - 1) / al * al;
    const size_t szr = ((size_t) n * 8 + al - 1) / al * al;
    /* the descriptors in perm order for the GCM kernels (GcmArgs::srecs) */
    const size_t szs = b.want_srecs ? ((size_t) n * sizeof(tlsrec_batch_rec) + al - 1) / al * al : 0;
    const size_t total = 2 * szk + szp + szr + szs + b.scan_bytes + al;
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
 *   tlsrec__test_fail_staging  the next n staging-area allocations of the
 *                              single-record engine fail (ALLOC_FAILED path)
 *   tlsrec__test_server_shadow served records read their key state from
 *                              copies at addresses whose low 32 bits have bit
 *                              31 set (the readfirstlane sign-extension case) */
#ifdef TLSREC_TEST_HOOKS
static volatile uint32_t g_test_skip = 0xffffffffu;
static volatile int g_test_fail_staging = 0;
static uint8_t *g_test_shadow = nullptr;
static size_t g_test_shadow_bytes = 0;

extern "C" void tlsrec__test_skip_record(uint32_t index) { g_test_skip = index; }
extern "C" void tlsrec__test_fail_staging(int n) { g_test_fail_staging = n; }
extern "C" void tlsrec__test_server_shadow(void *dev, size_t bytes)
{
    g_test_shadow = (uint8_t *) dev;
    g_test_shadow_bytes = dev ? bytes : 0;
}

/*   tlsrec__test_launch_log_*  the dispatchers' choices (tlsrec_internal.h
 *                              TLSREC_LAUNCH_LOG): the last LAUNCH_LOG_CAP
 *                              entries, oldest first */
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

extern "C" int tlsrec__server_yield(void);
extern "C" void tlsrec__server_note_batch(hipStream_t stream, int counted);

/* Launch options of one batch:
 *   only_mask  launch only these ciphers' kernels (1 << TLSREC_CIPHER_*; the
 *              single-record engine knows its records' ciphers), 0 = every
 *              cipher the table holds
 *   avg_bytes  mean record size when the caller knows it (the stream / DTLS
 *              layers, the host pipeline; 0 = unknown) -- it decides the GCM
 *              launch for many keys with little work each (below)
 *   prefilled  the caller already wrote INTERNAL_ERROR into every result (the
 *              single-record engine stages it with the upload)
 *   coalesced  a few records of many connections gathered from concurrent
 *              single-record calls: identity order (no bucket pass: its four
 *              launches would cost more than the batch), GCM in 16-lane wave
 *              passes, so each wave serves its own record's key */
struct BatchOpt {
    uint32_t only_mask = 0;
    uint32_t avg_bytes = 0;
    bool prefilled = false;
    bool coalesced = false;
    bool grouped = false;                /* a key's records are contiguous (the stream / DTLS layers: a connection's
                                            records in order): no bucket pass, the kernels walk them in place */
    const uint64_t *src_off = nullptr;   /* encrypt: contents at in + src_off[i] (tlsrec__batch_src) */
    bool no_cbc = false;                 /* the stream / DTLS layers without TLSREC_FRAME_CBC: a CBC slot counts as
                                            never loaded (no CBC kernel; its records get the bad-slot result) */
};

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

static int batch(const tlsrec_keytab *kt, const tlsrec_batch_rec *recs, tlsrec_batch_res *res, uint32_t n,
                 const uint8_t *in, uint8_t *out, uint32_t lanes, void *stream, int dec, const BatchOpt &opt = BatchOpt())
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


/* ======================================================================
 * Records in host memory: chunked H2D -> kernel -> D2H pipeline
 * (tlsrec_host_batch_*).  Records start and end in host socket buffers
 * (SURVEY.md 8(d)); a chunk is a run of consecutive records, its byte range
 * [buf_off of the first, end of the last) goes to one of NSLOT device slots,
 * is protected there in place, and comes back to the same offsets of the
 * output arena.  Three streams (H2D, kernels, D2H) chained by events keep
 * both copy directions and the kernels busy at once.
 * ==================================================================== */
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

static void host_pipe_free(HostPipe *p)
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

static int host_pipe_reserve(tlsrec_keytab *kt, size_t slot_bytes, size_t nrec)
{
    HostPipe *p = kt->pipe;
    if (!p) {
        p = new (std::nothrow) HostPipe();
        if (!p) return TLSREC_ERR_SSL_ALLOC_FAILED;
        kt->pipe = p;
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
    pthread_mutex_lock(&kt->pipe_mu);
    int rc = host_pipe_reserve(kt, (maxspan + 255) / 256 * 256, n);
    HostPipe *p = kt->pipe;
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
        if (zc) {
            /* the slot is free once its kernel is done */
            if (e == hipSuccess) e = hipStreamWaitEvent(p->d2h, p->ev_cmp[k], 0);
        } else {
            if (e == hipSuccess) e = hipStreamWaitEvent(p->d2h, p->ev_cmp[k], 0);
            if (e == hipSuccess) e = hipMemcpyAsync(out + C.base, p->slot[k], C.span, hipMemcpyDeviceToHost, p->d2h);
        }
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
    pthread_mutex_unlock(&kt->pipe_mu);
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

/* ======================================================================
 * Engine used by the single-record API (tlsrec_host.c).
 *
 * Key slots live in pages of ENGINE_PAGE_SLOTS (one key table each), added
 * as connections arrive -- ENGINE_MAX_PAGES x 4096 = 1 M slots, i.e. 512 K
 * connections per process.
 *
 * Concurrent calls are coalesced (flat combining, per page): a call queues
 * its record; if fewer than ENGINE_SETS batches of the page are in flight it
 * becomes the leader of the next one, takes every queued record (up to
 * ENGINE_BATCH, either direction), stages them in one pinned buffer, and runs
 * one H2D copy, one launch per direction and cipher (identity order: no
 * bucket pass), one D2H copy and one sync for all of them; the callers whose
 * records it carried are woken with their results.  A lone call is its own
 * leader: one record, one round trip.  Under load a round trip carries as
 * many records as arrived during the previous one.
 * ==================================================================== */
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
        /* zeroize (ssl_msg.c:6084-6099); the slot's cipher stays recorded in the
         * table's mask, so a later batch of this page may launch one kernel more.
         * A CBC slot needs no more than these three: its round keys of both
         * directions (rk / rkr / ark) lie in the SlotState, its HMAC midstates at
         * the head of the table area. */
        hipMemsetAsync(kt->d_slots + i, 0, sizeof(SlotState), g_load);
        hipMemsetAsync(kt->d_cipher + i, 0, 1, g_load);
        hipMemsetAsync(kt->d_ghtab + (size_t) i * KEY_TABLE_WORDS, 0, sizeof(uint4) * KEY_TABLE_WORDS, g_load);
        /* (the GHASH tables end with H^1..H^64, the record server's closing powers) */
        hipStreamSynchronize(g_load);
        kt->h_cipher[i] = 0;
        kt->nloaded--;
        P->used[i] = 0;
        P->etm[i] = 0;
        P->nused--;
    }
    pthread_mutex_unlock(&g_mu);
}

#ifdef TLSREC_TEST_HOOKS
/* test hook: the device bytes of an engine slot -- its SlotState (1024 B),
 * the first 1024 B of its GHASH tables and its 64 record-server powers
 * (1024 B) -- copied to host, to show what slot_free leaves behind */
extern "C" int tlsrec__test_engine_slot_dump(int slot, void *state, void *ghtab, void *hpw)
{
    pthread_mutex_lock(&g_mu);
    uint32_t i = 0;
    tlsrec_keytab *kt = slot_table(slot, &i);
    int r = kt ? 0 : TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!r && (hipMemcpy(state, kt->d_slots + i, sizeof(SlotState), hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemcpy(ghtab, kt->d_ghtab + (size_t) i * KEY_TABLE_WORDS, 1024, hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemcpy(hpw, kt->d_ghtab + (size_t) i * KEY_TABLE_WORDS + KEY_HPOW_OFF, 1024,
                         hipMemcpyDeviceToHost) != hipSuccess))
        r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
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

static size_t al(size_t x, size_t a) { return (x + a - 1) / a * a; }

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
    const size_t off_res = al((size_t) n * sizeof(tlsrec_batch_rec), 256);
    const size_t off_arena = al(off_res + (size_t) n * sizeof(tlsrec_batch_res), 256);
    size_t used = 0;
    size_t boff[ENGINE_BATCH];
    for (uint32_t i = 0; i < n; i++) {
        boff[i] = used;
        used = al(used + v[i]->buf_len + v[i]->d.cid_len + 16, ENGINE_ALIGN);
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

/* server.hip: the resident record server (AES-GCM, ChaCha20-Poly1305) */
extern "C" int tlsrec__server_run(int dec, uint32_t cipher, uint32_t nr, const tlsrec_batch_rec *rec,
                                  const void *slot_state, const void *ghtab, const void *hpw, unsigned char *buf,
                                  size_t buf_len, const void *plan, int skip, tlsrec_batch_res *out);

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
    const uint32_t cipher = kt->h_cipher[idx];
    if (cipher == 0) return TLSREC_ERR_SSL_INTERNAL_ERROR;
    if (buf_len > 0xffffffffu - 64) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    /* per slot, not the page's has_cid: one CID connection must not take the
     * server away from the page's other 4095 slots */
    if ((tlsrec_cipher_is_gcm((int) cipher) || cipher == TLSREC_CIPHER_CHACHA20_POLY1305) &&
        !g_pages[rec->slot / ENGINE_PAGE_SLOTS].cid[idx] && rec->cid_len == 0) {
        tlsrec_batch_rec d = *rec;
        d.slot = idx;
        const void *p_state = kt->d_slots + idx;
        const void *p_ghtab = kt->d_ghtab + (size_t) idx * KEY_TABLE_WORDS;
        const void *p_hpw = kt->d_ghtab + (size_t) idx * KEY_TABLE_WORDS + KEY_HPOW_OFF;
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
                                         buf, buf_len, plan, g_test_skip == 0, out);
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

/* the same for one queue (engine_queue: family * 2 + direction; families GCM, ChaCha20-Poly1305, CCM, CBC) */
extern "C" int tlsrec__engine_queue_stats(int queue, uint64_t *batches, uint64_t *records)
{
    if (queue < 0 || queue >= ENGINE_QUEUES) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    uint64_t b = 0, r = 0;
    for (int pg = 0; pg < g_npages; pg++) {
        Combiner *c = g_pages[pg].co[queue];
        if (!c) continue;
        pthread_mutex_lock(&c->mu);
        b += c->batches;
        r += c->records;
        pthread_mutex_unlock(&c->mu);
    }
    if (batches) *batches = b;
    if (records) *records = r;
    return 0;
}

/* coalescing statistics over every page: batches run and records carried */
extern "C" void tlsrec__engine_stats(uint64_t *batches, uint64_t *records)
{
    uint64_t b = 0, r = 0;
    for (int pg = 0; pg < g_npages; pg++)
        for (int q = 0; q < ENGINE_QUEUES; q++) {
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
