/*
 * keytab.hip -- the key table: device memory of the slots, the loads that fill them, and the bookkeeping
 * (tlsrec_keytab.h) the launches are sized from.
 *
 * Plain HIP runtime C++ behind the extern "C" ABI of include/tlsrec.h: no kernel here, the key setup runs in
 * kernels.hip, cbc.hip and cbc_alt.hip.
 */
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_cbc.h"
#include "tlsrec_frame.h"
#include "tlsrec_internal.h"
#include "tlsrec_keytab.h"

using namespace tlsrec;

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

extern "C" void tlsrec_keytab_free(tlsrec_keytab *kt)
{
    if (!kt) return;
    tlsrec__host_pipe_free(kt->pipe);
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

extern "C" uint32_t tlsrec_keytab_capacity(const tlsrec_keytab *kt) { return kt ? kt->capacity : 0; }

extern "C" int tlsrec__keytab_cipher(const tlsrec_keytab *kt, uint32_t slot)
{
    return kt && slot < kt->capacity ? kt->h_cipher[slot] : 0;
}
extern "C" const SlotState *tlsrec__keytab_slots(const tlsrec_keytab *kt) { return kt->d_slots; }
extern "C" const uint4 *tlsrec__keytab_ghtab(const tlsrec_keytab *kt) { return kt->d_ghtab; }

HostPipe **tlsrec__keytab_pipe_lock(tlsrec_keytab *kt)
{
    pthread_mutex_lock(&kt->pipe_mu);
    return &kt->pipe;
}
void tlsrec__keytab_pipe_unlock(tlsrec_keytab *kt) { pthread_mutex_unlock(&kt->pipe_mu); }

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

/* zeroize (ssl_msg.c:6084-6099).  A CBC slot needs no more than these three: its round keys of both
 * directions (rk / rkr / ark) lie in the SlotState, its HMAC midstates at the head of the table area (which
 * ends with H^1..H^64, the record server's closing powers). */
void tlsrec__keytab_slot_zeroize(tlsrec_keytab *kt, uint32_t slot, hipStream_t st)
{
    hipMemsetAsync(kt->d_slots + slot, 0, sizeof(SlotState), st);
    hipMemsetAsync(kt->d_cipher + slot, 0, 1, st);
    hipMemsetAsync(kt->d_ghtab + (size_t) slot * KEY_TABLE_WORDS, 0, sizeof(uint4) * KEY_TABLE_WORDS, st);
    hipStreamSynchronize(st);
    kt->clear(slot);
}

/* ---- loading key material ----
 * tlsrec_keytab_load and tlsrec_keytab_load_cbc follow one sequence: arguments, fetch (device-resident material
 * comes to the host for the checks), check, stage (host material goes to the device for the kernel), bookkeeping,
 * key setup, cleanup.  Nothing is noted in the book before every record has passed its check. */

/* `count` records of device-resident material on the host; *host is NULL on an error, else the caller's to
 * wipe_free */
template <class K> static int fetch_material(const K *keys, uint32_t count, hipStream_t st, K **host)
{
    const size_t bytes = sizeof(K) * (size_t) count;
    *host = (K *) malloc(bytes);
    if (!*host) return TLSREC_ERR_SSL_ALLOC_FAILED;
    if (hipMemcpyAsync(*host, keys, bytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
        hipStreamSynchronize(st) == hipSuccess)
        return 0;
    free(*host);
    *host = NULL;
    return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

/* `count` records of host material at `dst` on the device; the copy has landed on return, so the caller's
 * buffer may be reused */
template <class K> static int stage_material(K *dst, const K *keys, uint32_t count, hipStream_t st)
{
    return hipMemcpyAsync(dst, keys, sizeof(K) * (size_t) count, hipMemcpyHostToDevice, st) == hipSuccess &&
                   hipStreamSynchronize(st) == hipSuccess
               ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}

/* the fetched copy holds raw keys */
template <class K> static void wipe_free(K *host, uint32_t count)
{
    if (!host) return;
    memset(host, 0, sizeof(K) * (size_t) count);
    free(host);
}

/* A slot that held a CBC key and now gets an AEAD one: its round keys of both
 * directions (SlotState::rk / rkr and ark, whichever way its cipher lays them
 * out) and HMAC midstates (the head of its table area) are not all
 * overwritten by the AEAD key setup, so one kernel zeroizes them,
 * enqueued before the key setup (a table that never held a CBC key: nothing). */
static int aead_keysetup(tlsrec_keytab *kt, const tlsrec_key_material *src, uint32_t first, uint32_t count,
                         hipStream_t st)
{
    if ((kt->cipher_mask & CBC_CIPHER_BITS) &&
        tlsrec__launch_cbc_wipe(kt->d_slots, kt->d_ghtab, kt->d_cipher, first, count, st) != hipSuccess)
        return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    return hip_ok(tlsrec__launch_keysetup(kt->d_slots, kt->d_ghtab, kt->d_cipher, src, first, count, st));
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
    if (!kt || !keys || !kt->holds(first, count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    tlsrec_key_material *host = NULL;
    int r = keys_on_device ? fetch_material(keys, count, st, &host) : 0;
    const tlsrec_key_material *hk = keys_on_device ? host : keys;
    for (uint32_t i = 0; i < count && !r; i++) r = check_material(&hk[i]);
    if (!r && !keys_on_device) r = stage_material(kt->d_stage + first, keys, count, st);
    if (!r) {
        for (uint32_t i = 0; i < count; i++) kt->note(first + i, 1, hk[i].cipher);
        r = aead_keysetup(kt, keys_on_device ? keys : kt->d_stage + first, first, count, st);
    }
    wipe_free(host, count);
    return r;
}

static int check_cbc_material(const tlsrec_cbc_key_material *k, uint32_t count)
{
    for (uint32_t i = 0; i < count; i++) {
        /* unknown cipher or MAC, or an ARIA / Camellia id with a MAC no suite pairs it with */
        if (!cbc_pair_ok(k[i].cipher, k[i].mac)) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
        if (k[i].tls_minor != 3 || k[i].etm > 1) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    }
    return 0;
}

/* Key setup of `count` checked CBC records (hk: their host copy, dk: the device copy the kernels read): one
 * launch per run of records of one kind (AES / ARIA or Camellia), so neither kernel meets the other's material */
static int cbc_keysetup_runs(tlsrec_keytab *kt, const tlsrec_cbc_key_material *hk, const tlsrec_cbc_key_material *dk,
                             uint32_t first, uint32_t count, hipStream_t st)
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

extern "C" int tlsrec_keytab_load_cbc(tlsrec_keytab *kt, uint32_t first, uint32_t count,
                                      const tlsrec_cbc_key_material *keys, int keys_on_device, void *stream)
{
    /* the one step out of order: host material is judged before the arguments -- its errors need neither a
     * table nor a device, and a caller that passes both bad gets the material's */
    int r = keys && !keys_on_device ? check_cbc_material(keys, count) : 0;
    if (r) return r;
    if (!kt || !keys || !kt->holds(first, count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    const size_t bytes = sizeof(*keys) * (size_t) count;
    tlsrec_cbc_key_material *host = NULL, *dev = NULL;
    if (keys_on_device) {
        r = fetch_material(keys, count, st, &host);
        if (!r) r = check_cbc_material(host, count);
    } else if (hipMalloc((void **) &dev, bytes) != hipSuccess) {
        /* 128-byte records with raw MAC keys: a staging buffer of this call's own, not one that outlives it */
        r = TLSREC_ERR_SSL_ALLOC_FAILED;
    } else {
        r = stage_material(dev, keys, count, st);
    }
    if (!r) {
        const tlsrec_cbc_key_material *hk = keys_on_device ? host : keys;
        for (uint32_t i = 0; i < count; i++) kt->note_cbc(first + i, 1, hk[i].cipher, hk[i].mac, hk[i].etm);
        r = cbc_keysetup_runs(kt, hk, keys_on_device ? keys : dev, first, count, st);
    }
    wipe_free(host, count);
    if (dev) {
        /* the staged copy holds raw keys: wait for the kernel, zeroize, free */
        hipStreamSynchronize(st);
        hipMemset(dev, 0, bytes);
        hipFree(dev);
    }
    return r;
}

/* Device-side producers of key material (keysched.hip, tls13_ladder.hip, tls12_batch.hip) write into the
 * table's staging area and then commit: bookkeeping as tlsrec_keytab_load,
 * then the key-setup kernel on the staged slots. */
extern "C" tlsrec_key_material *tlsrec__keytab_stage(tlsrec_keytab *kt) { return kt->d_stage; }

extern "C" int tlsrec__keytab_commit_staged(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                            hipStream_t st)
{
    kt->note(first, count, cipher);
    return aead_keysetup(kt, kt->d_stage + first, first, count, st);
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
    kt->note_cbc(first, count, cipher, mac, etm);
    tlsrec_cbc_key_material *src = kt->d_stage_cbc + first;
    int r = hip_ok(tlsrec__launch_cbc_keysetup(kt->d_slots, kt->d_ghtab, kt->d_cipher, src, first, count,
                                               cbc_is_alt(cipher), st));
    if (hipMemsetAsync(src, 0, sizeof(*src) * (size_t) count, st) != hipSuccess && r == 0)
        r = TLSREC_ERR_SSL_HW_ACCEL_FAILED;
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
