/*
 * tls13_ladder.hip -- the TLS 1.3 key-schedule ladder in batches, one
 * connection per lane, on the word-wise blocks of tlsrec_kdf.h
 * (library/ssl_tls13_keys.c, ssl_tls13_server.c):
 *
 *   reference                                   here
 *   ..._derive_early / _handshake / _application_secrets :421-650,
 *   ssl_tls13_calc_finished_core        :697    tlsrec_tls13_keytab_derive_handshake, _application,
 *                                               tlsrec_tls13_batch_verify_data, _batch_derive_secret:
 *                                               the ladder from PSK / (EC)DHE secret to the application
 *                                               keys, written for its fixed shapes like the TLS 1.2 batch
 *   ssl_tls13_offered_psks_check_binder_match
 *                  (ssl_tls13_server.c:404-457)  tlsrec_tls13_batch_psk_binder
 *   ssl_tls13_generate_early_key :1086-1182,
 *   ..._compute_early_transform  :1184-1225     tlsrec_tls13_keytab_derive_early
 *   the "resumption" Expand-Label
 *                (ssl_tls13_server.c:3219-3230)  tlsrec_tls13_batch_ticket_psk
 *
 * The single-shot forms of the same steps are in keysched.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "tlsrec.h"
#include "tlsrec_frame.h"     /* tlsrec_cipher_keylen, tlsrec_cipher_taglen */
#include "tlsrec_internal.h"
#include "tlsrec_kdf.h"

namespace tlsks {

/* ---------------- TLS 1.3 ladder, batch ----------------------------------
 * Early Secret -> Handshake Secret -> handshake traffic keys and Finished
 * keys -> Master Secret -> application traffic keys (RFC 8446 7.1; the helpers
 * of ssl_tls13_keys.c:421-650 and ssl_tls13_calc_finished_core :697), one
 * connection per lane.  As in the TLS 1.2 kernels nothing goes through a
 * byte-wise hash: every message here is a single inner block whose words are put
 * together with constant indices -- an HkdfLabel with a label of at most 12
 * characters and a context of H bytes, || 0x01, is at most 55 bytes (SHA-256)
 * or 71 (SHA-384) -- except the Extract over a 56- or 66-byte shared secret
 * under SHA-256, which takes a second one.  The HMAC midstates of a secret are
 * computed once and serve every Expand under it; the midstates of the zero
 * salt, Hash("") and, for a connection without a PSK, the midstates of
 * Derive-Secret(Early Secret, "derived", "") are the same for every connection
 * and arrive as kernel arguments (LadderConsts, scalar registers).
 *
 * Messages are addressed in 32-bit big-endian cells: 16 to a SHA-256 block, 32
 * to a SHA-512 one. */

/* the labels of one stage, each with its Hash.length / key length / 12 as the
 * output length and the context length it is used with */
struct LadderLabels { LabelW derived, c_traffic, s_traffic, extra, key, iv, fin; };
enum { OFF_DERIVED = 17, OFF_TRAFFIC = 22, OFF_EXP_MASTER = 20, OFF_KEY = 13, OFF_IV = 12, OFF_FINISHED = 18 };

/* One direction under its traffic secret ts: write_key, write_iv
 * (ssl_tls13_make_traffic_key, ssl_tls13_keys.c:219-246) as a
 * tlsrec_key_material, and the Finished key if fin != NULL.  2 + 4 (+ 2)
 * compressions. */
template <class T>
__device__ __forceinline__ void traffic_side(const typename T::W (&ts)[T::HW], const LadderLabels &lb, uint32_t head,
                                             uint32_t key_cells, tlsrec_key_material *km_dst, tlsrec_tls13_secret *fin,
                                             bool fin_aligned)
{
    typedef typename T::W W;
    W ip[8], op[8], w[16], K[T::HW], V[T::HW];
    hmac_mid<T>(ts, ip, op);
    label_block<T, OFF_KEY, false>(w, lb.key, K);
    hmac_block<T>(ip, op, w, K);
    label_block<T, OFF_IV, false>(w, lb.iv, V);
    hmac_block<T>(ip, op, w, V);
    uint32_t km[16];
    km[0] = head;
#pragma unroll
    for (int j = 1; j < 16; j++) km[j] = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) km[4 + j] = __builtin_bswap32(cell<T, T::HW>(V, j));
#pragma unroll
    for (int j = 0; j < 8; j++) km[8 + j] = (uint32_t) j < key_cells ? __builtin_bswap32(cell<T, T::HW>(K, j)) : 0u;
    uint4 *dst = reinterpret_cast<uint4 *>(km_dst);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = make_uint4(km[4 * k], km[4 * k + 1], km[4 * k + 2], km[4 * k + 3]);
    if (fin) {
        label_block<T, OFF_FINISHED, false>(w, lb.fin, K);
        hmac_block<T>(ip, op, w, K);
        store_secret<T>(fin, fin_aligned, K);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) km[j] = 0;
#pragma unroll
    for (int j = 0; j < T::HW; j++) { K[j] = 0; V[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
}

template <class T> struct Tls13HsArgs {
    const tlsrec_tls13_hs_conn *conns;
    tlsrec_key_material *out;             /* staging area of slot `first`: 2 records per connection */
    tlsrec_tls13_secret *hs_traffic, *finished, *master;
    uint32_t count, head, key_cells, psk_len, shared_len, aligned;
    LadderConsts<T> k;
    LadderLabels lb;
};

/* Compressions per connection: no PSK 0, a PSK 8 (Extract 2,
 * midstates 2, "derived" 2, midstates 2); Extract over the shared secret 2 (3
 * for 56 / 66 bytes under SHA-256); midstates 2; two traffic secrets 4;
 * "derived" 2, midstates 2, Master Secret 2; each direction 2 + key 2 + iv 2 +
 * finished 2: 30 / 38 with both Finished keys, 26 / 34 without. */
template <class T> __global__ void __launch_bounds__(64) tls13_hs_kernel(Tls13HsArgs<T> a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint8_t *conn = reinterpret_cast<const uint8_t *>(a.conns + i);
    const bool cal = (a.aligned & AL_CONNS) != 0;
    W ip[8], op[8], w[16], x[T::HW];
    if (a.psk_len) {
        /* Early Secret = Extract(0, PSK); then the salt of the next Extract */
        uint32_t P[12];
        load_cells<12>(conn, cal, P);
        msg_block<T, 12>(w, P, a.psk_len, 0);
        hmac_block<T>(a.k.zero_ip, a.k.zero_op, w, x);
        hmac_mid<T>(x, ip, op);
        label_block<T, OFF_DERIVED, true>(w, a.lb.derived, a.k.empty);
        hmac_block<T>(ip, op, w, x);
        hmac_mid<T>(x, ip, op);
#pragma unroll
        for (int j = 0; j < 12; j++) P[j] = 0;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) { ip[j] = a.k.d0_ip[j]; op[j] = a.k.d0_op[j]; }
    }
    /* Handshake Secret = Extract(., shared), H zero bytes for psk_ke */
    {
        W st[8];
#pragma unroll
        for (int j = 0; j < 8; j++) st[j] = ip[j];
        if (a.shared_len) {
            uint32_t Sh[20];
            load_cells<20>(conn + 48, cal, Sh);
            msg_block<T, 20>(w, Sh, a.shared_len, 0);
            sha_compress<typename T::S>(st, w);
            if (a.shared_len + 1 + T::LENB > T::BB) {
                msg_block<T, 20>(w, Sh, a.shared_len, 1);
                sha_compress<typename T::S>(st, w);
            }
#pragma unroll
            for (int j = 0; j < 20; j++) Sh[j] = 0;
        } else {
#pragma unroll
            for (int j = 0; j < T::HW; j++) x[j] = 0;
            digest_block<T>(w, x);
            sha_compress<typename T::S>(st, w);
        }
        hmac_outer<T>(op, st, x);
    }
    hmac_mid<T>(x, ip, op);
    W tr[T::HW], cs[T::HW], ss[T::HW];
    load_digest<T>(conn + 128, cal, tr);
    label_block<T, OFF_TRAFFIC, true>(w, a.lb.c_traffic, tr);
    hmac_block<T>(ip, op, w, cs);
    label_block<T, OFF_TRAFFIC, true>(w, a.lb.s_traffic, tr);
    hmac_block<T>(ip, op, w, ss);
    /* Master Secret = Extract(Derive-Secret(Handshake Secret, "derived", ""), 0) */
    label_block<T, OFF_DERIVED, true>(w, a.lb.derived, a.k.empty);
    hmac_block<T>(ip, op, w, x);
    hmac_mid<T>(x, ip, op);
#pragma unroll
    for (int j = 0; j < T::HW; j++) x[j] = 0;
    digest_block<T>(w, x);
    hmac_block<T>(ip, op, w, x);
    store_secret<T>(a.master + i, (a.aligned & AL_MASTER) != 0, x);
    store_secret<T>(a.hs_traffic + 2 * (size_t) i, (a.aligned & AL_TRAFFIC) != 0, cs);
    store_secret<T>(a.hs_traffic + 2 * (size_t) i + 1, (a.aligned & AL_TRAFFIC) != 0, ss);
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
#pragma unroll
        for (int j = 0; j < T::HW; j++) x[j] = side ? ss[j] : cs[j];
        traffic_side<T>(x, a.lb, a.head, a.key_cells, a.out + 2 * (size_t) i + side,
                        a.finished ? a.finished + 2 * (size_t) i + side : nullptr, (a.aligned & AL_AUX) != 0);
    }
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; cs[j] = 0; ss[j] = 0; tr[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

template <class T> struct Tls13AppArgs {
    const tlsrec_tls13_secret *master, *transcripts;
    tlsrec_key_material *out;
    tlsrec_tls13_secret *app_traffic, *exporter;
    uint32_t count, head, key_cells, aligned;
    LadderLabels lb;                      /* extra: "exp master" */
};

/* Compressions per connection: midstates 2, two traffic secrets 4, exporter
 * master secret 2, each direction 2 + key 2 + iv 2: 20, 18 without the exporter. */
template <class T> __global__ void __launch_bounds__(64) tls13_app_kernel(Tls13AppArgs<T> a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8], w[16], x[T::HW], tr[T::HW], cs[T::HW], ss[T::HW];
    load_digest<T>(a.master[i].secret, (a.aligned & AL_MASTER) != 0, x);
    load_digest<T>(a.transcripts[i].secret, (a.aligned & AL_TRANSCRIPT) != 0, tr);
    hmac_mid<T>(x, ip, op);
    label_block<T, OFF_TRAFFIC, true>(w, a.lb.c_traffic, tr);
    hmac_block<T>(ip, op, w, cs);
    label_block<T, OFF_TRAFFIC, true>(w, a.lb.s_traffic, tr);
    hmac_block<T>(ip, op, w, ss);
    if (a.exporter) {
        label_block<T, OFF_EXP_MASTER, true>(w, a.lb.extra, tr);
        hmac_block<T>(ip, op, w, x);
        store_secret<T>(a.exporter + i, (a.aligned & AL_AUX) != 0, x);
    }
    store_secret<T>(a.app_traffic + 2 * (size_t) i, (a.aligned & AL_TRAFFIC) != 0, cs);
    store_secret<T>(a.app_traffic + 2 * (size_t) i + 1, (a.aligned & AL_TRAFFIC) != 0, ss);
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
#pragma unroll
        for (int j = 0; j < T::HW; j++) x[j] = side ? ss[j] : cs[j];
        traffic_side<T>(x, a.lb, a.head, a.key_cells, a.out + 2 * (size_t) i + side, nullptr, false);
    }
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; cs[j] = 0; ss[j] = 0; tr[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* out[i] = HMAC(keys[i], msgs[i]) over H-byte messages (verify_data under a
 * Finished key), or with label_len != ~0u Expand-Label(keys[i], label, msgs[i], H)
 * (Derive-Secret with a hashed context): 4 compressions either way. */
struct Tls13MacArgs {
    const tlsrec_tls13_secret *keys, *msgs;
    tlsrec_tls13_secret *out;
    uint32_t count, aligned, label_len;   /* AL_MASTER keys, AL_TRANSCRIPT msgs, AL_AUX out */
    LabelW label;
};
enum : uint32_t { MAC_PLAIN = ~0u };

template <class T> __global__ void __launch_bounds__(64) tls13_mac_kernel(Tls13MacArgs a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8], w[16], x[T::HW], m[T::HW];
    load_digest<T>(a.keys[i].secret, (a.aligned & AL_MASTER) != 0, x);
    load_digest<T>(a.msgs[i].secret, (a.aligned & AL_TRANSCRIPT) != 0, m);
    hmac_mid<T>(x, ip, op);
    /* the label's length only moves the context inside the block: wave-uniform */
    switch (a.label_len) {
        case 0: label_block<T, 10, true>(w, a.label, m); break;
        case 1: label_block<T, 11, true>(w, a.label, m); break;
        case 2: label_block<T, 12, true>(w, a.label, m); break;
        case 3: label_block<T, 13, true>(w, a.label, m); break;
        case 4: label_block<T, 14, true>(w, a.label, m); break;
        case 5: label_block<T, 15, true>(w, a.label, m); break;
        case 6: label_block<T, 16, true>(w, a.label, m); break;
        case 7: label_block<T, 17, true>(w, a.label, m); break;
        case 8: label_block<T, 18, true>(w, a.label, m); break;
        case 9: label_block<T, 19, true>(w, a.label, m); break;
        case 10: label_block<T, 20, true>(w, a.label, m); break;
        case 11: label_block<T, 21, true>(w, a.label, m); break;
        case 12: label_block<T, 22, true>(w, a.label, m); break;
        default: digest_block<T>(w, m); break;
    }
    hmac_block<T>(ip, op, w, x);
    store_secret<T>(a.out + i, (a.aligned & AL_AUX) != 0, x);
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; m[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* ---- a resumed handshake: PSK binder, 0-RTT keys, ticket PSK ---------------
 * An HkdfLabel up to and including its context-length byte is 2 (length) + 1
 * (label length) + 6 ("tls13 ") + the label + 1 bytes, so the context starts
 * at 10 + strlen(label): "res binder" / "ext binder" (10 characters) 20,
 * "c e traffic" (11) 21, "e exp master" (12) 22, "resumption" (10) 20. */
enum { OFF_BINDER = 20, OFF_E_TRAFFIC = 21, OFF_E_EXP_MASTER = 22, OFF_RESUMPTION = 20 };
enum { AL_BINDERS = AL_MASTER, AL_OFFERED = AL_TRANSCRIPT };

template <class T> struct Tls13EarlyArgs {
    const tlsrec_tls13_psk_conn *conns;
    const tlsrec_tls13_secret *offered;   /* with match, or both NULL */
    tlsrec_tls13_secret *binders;         /* may be NULL */
    uint32_t *match;
    tlsrec_key_material *out;             /* staging area of slot `first`, one record per connection; NULL: binder only */
    tlsrec_tls13_secret *early_traffic, *early_exporter;    /* read only with out; early_exporter may be NULL */
    uint32_t count, head, key_cells, psk_len, aligned;
    LadderConsts<T> k;
    LabelW binder, c_e, e_exp;            /* "res binder" or "ext binder", "c e traffic", "e exp master" */
    LadderLabels lb;                      /* key, iv, fin */
};

/* ssl_tls13_offered_psks_check_binder_match (ssl_tls13_server.c:404-457) and,
 * with a.out, ssl_tls13_generate_early_key (ssl_tls13_keys.c:1086-1182), one
 * connection per lane.  Compressions per connection: the binder
 * 14 (Extract 2, midstates 2, binder key 2, midstates 2, finished key 2,
 * midstates 2, MAC 2; the Early Secret's midstates also serve the early
 * secrets); the early keys 10 more (two secrets 4, midstates 2, key 2, iv 2),
 * 8 without the exporter: 14 / 22 / 24.  The two early secrets come before the
 * binder key's midstates so that one pair of midstates is live at a time. */
template <class T> __global__ void __launch_bounds__(64) tls13_early_kernel(Tls13EarlyArgs<T> a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint8_t *conn = reinterpret_cast<const uint8_t *>(a.conns + i);
    const bool cal = (a.aligned & AL_CONNS) != 0;
    W ip[8], op[8], w[16], x[T::HW], tr[T::HW], cs[T::HW];
    {
        /* Early Secret = Extract(0, PSK) */
        uint32_t P[12];
        load_cells<12>(conn, cal, P);
        msg_block<T, 12>(w, P, a.psk_len, 0);
        hmac_block<T>(a.k.zero_ip, a.k.zero_op, w, x);
#pragma unroll
        for (int j = 0; j < 12; j++) P[j] = 0;
    }
    hmac_mid<T>(x, ip, op);
    if (a.out) {
        load_digest<T>(conn + 96, cal, tr);
        label_block<T, OFF_E_TRAFFIC, true>(w, a.c_e, tr);
        hmac_block<T>(ip, op, w, cs);
        store_secret<T>(a.early_traffic + i, (a.aligned & AL_TRAFFIC) != 0, cs);
        if (a.early_exporter) {
            label_block<T, OFF_E_EXP_MASTER, true>(w, a.e_exp, tr);
            hmac_block<T>(ip, op, w, x);
            store_secret<T>(a.early_exporter + i, (a.aligned & AL_AUX) != 0, x);
        }
    }
    /* binder_key = Derive-Secret(Early Secret, "res binder" | "ext binder", ""), then
     * ssl_tls13_calc_finished_core over the truncated ClientHello's hash */
    label_block<T, OFF_BINDER, true>(w, a.binder, a.k.empty);
    hmac_block<T>(ip, op, w, x);
    hmac_mid<T>(x, ip, op);
    label_block<T, OFF_FINISHED, false>(w, a.lb.fin, x);
    hmac_block<T>(ip, op, w, x);
    hmac_mid<T>(x, ip, op);
    load_digest<T>(conn + 48, cal, tr);
    digest_block<T>(w, tr);
    hmac_block<T>(ip, op, w, x);
    if (a.binders) store_secret<T>(a.binders + i, (a.aligned & AL_BINDERS) != 0, x);
    if (a.match) {
        /* mbedtls_ct_memcmp: the OR of the XOR of every cell, no early exit, no branch on the data */
        load_digest<T>(a.offered[i].secret, (a.aligned & AL_OFFERED) != 0, tr);
        W d = 0;
#pragma unroll
        for (int j = 0; j < T::HW; j++) d |= x[j] ^ tr[j];
        uint32_t d32 = (uint32_t) d;
        if constexpr (sizeof(W) == 8) d32 |= (uint32_t) ((uint64_t) d >> 32);
        a.match[i] = d32 == 0 ? 1u : 0u;
    }
    if (a.out) traffic_side<T>(cs, a.lb, a.head, a.key_cells, a.out + i, nullptr, false);
#pragma unroll
    for (int j = 0; j < T::HW; j++) { x[j] = 0; tr[j] = 0; cs[j] = 0; }
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

/* psk[i] = HKDF-Expand-Label(res_master[i], "resumption", nonce i, H)
 * (ssl_tls13_server.c:3219-3230): 4 compressions.  The 20 bytes of the
 * HkdfLabel up to its context-length byte fill cells 0..4, so the nonce starts
 * on cell 5; its length is wave-uniform, and the 0x01 that closes the
 * HkdfLabel, the 0x80 and the length word (msg_block) move with it. */
struct Tls13TicketArgs {
    const tlsrec_tls13_secret *res_master;
    const uint8_t *nonces;                /* 32 bytes per ticket, nonce_len used */
    tlsrec_tls13_secret *psk;
    uint32_t count, aligned, nonce_len;   /* AL_MASTER res_master, AL_TRANSCRIPT nonces, AL_AUX psk */
    LabelW label;
};

template <class T> __global__ void __launch_bounds__(64) tls13_ticket_kernel(Tls13TicketArgs a)
{
    typedef typename T::W W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    W ip[8], op[8], w[16], x[T::HW];
    load_digest<T>(a.res_master[i].secret, (a.aligned & AL_MASTER) != 0, x);
    hmac_mid<T>(x, ip, op);
    uint32_t N[8], m[14];
    load_cells<8>(a.nonces + 32 * (size_t) i, (a.aligned & AL_TRANSCRIPT) != 0, N);
#pragma unroll
    for (int c = 0; c < 5; c++) m[c] = a.label.c[c];
#pragma unroll
    for (int c = 0; c < 9; c++) {
        const int rem = (int) a.nonce_len - 4 * c;          /* nonce bytes from this cell on */
        const uint32_t v = c < 8 ? N[c] : 0u;
        uint32_t y;
        if (rem >= 4) y = v;
        else if (rem >= 0) y = (rem ? v & ~(0xffffffffu >> (8 * rem)) : 0u) | (0x01u << (24 - 8 * rem));
        else y = 0u;
        m[5 + c] = y;
    }
    msg_block<T, 14>(w, m, OFF_RESUMPTION + a.nonce_len + 1, 0);
    hmac_block<T>(ip, op, w, x);
    store_secret<T>(a.psk + i, (a.aligned & AL_AUX) != 0, x);
#pragma unroll
    for (int j = 0; j < 8; j++) N[j] = 0;
#pragma unroll
    for (int j = 0; j < 14; j++) m[j] = 0;
#pragma unroll
    for (int j = 0; j < T::HW; j++) x[j] = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { ip[j] = 0; op[j] = 0; }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
}

} /* namespace tlsks */

using namespace tlsks;

/* ---- the ladder in batches (tls13_hs_kernel, tls13_app_kernel, tls13_mac_kernel) ---- */
/* HMAC midstates of the zero salt, of Derive-Secret(Extract(0, 0), "derived", ""),
 * and Hash(""): tests/tls13_ref.py ladder_constants() computes them from FIPS 180-4
 * and hashlib, tests/test_tls13_ladder_cpu.py compares. */
static const LadderConsts<L256> kConsts256 = {
    { 0xf454deadu, 0x9725214fu, 0x90daf2a0u, 0xdf1228eau, 0x64e5750fu, 0xa3924181u, 0x824a932bu, 0xf8e04e32u },
    { 0xd385480fu, 0x7abb6477u, 0x37c9c538u, 0x5dd82467u, 0x8e043a72u, 0x753434b0u, 0xdeb82818u, 0x361d45a6u },
    { 0x8b35051cu, 0x8324ce6fu, 0xd35fd442u, 0x05006b0bu, 0x11f653deu, 0x87170024u, 0x53923a72u, 0x1a2e89f5u },
    { 0x22b91d2fu, 0xa7f9ba55u, 0xba705a48u, 0xa6bef047u, 0xf5ba9b91u, 0xc425b796u, 0xdb8072a6u, 0x9037dbc2u },
    { 0xe3b0c442u, 0x98fc1c14u, 0x9afbf4c8u, 0x996fb924u, 0x27ae41e4u, 0x649b934cu, 0xa495991bu, 0x7852b855u } };
static const LadderConsts<L384> kConsts384 = {
    { 0x53f869327560c3a2ULL, 0xc237b05164a5bbe8ULL, 0xe581f7394cfa66b8ULL, 0x846fa61922faad62ULL,
      0xdd0b37ce462cff5eULL, 0x7ee8a4bdc87567f3ULL, 0x39bda99c75a047f7ULL, 0xc7bd628bd3f9a734ULL },
    { 0xff6ce3f9ca86c81cULL, 0x585559c2ae0fc15cULL, 0xcf0d5686fb65a54eULL, 0xf1d54ee19e8cfd02ULL,
      0xa5c720ab778ff100ULL, 0xdeb3e5f667573e8cULL, 0xc1bfc7ec16b591f3ULL, 0x34d487c1c79d59ebULL },
    { 0x9540faa284271b10ULL, 0x940f9b21f2567a8cULL, 0x43d6380a7b89a867ULL, 0xedb7635f9865feb1ULL,
      0x7c8b33059f3e823eULL, 0x9eb66f676065f021ULL, 0x79f7d919bede4e6dULL, 0x80ad994f8a39c726ULL },
    { 0x9dcd6bc600f811e3ULL, 0xc556680dbba9586eULL, 0x987fb78efb62dcb7ULL, 0xb639835d0b42573aULL,
      0x81cf02b2e173ad99ULL, 0x30a7f1029298d495ULL, 0x8aa72679937f7672ULL, 0xd31f72c4ad9a4b4cULL },
    { 0x38b060a751ac9638ULL, 0x4cd9327eb1b1e36aULL, 0x21fdb71114be0743ULL, 0x4c0cc7bf63f6e1daULL,
      0x274edebfe76f65fbULL, 0xd51ad2f14898b95bULL } };

template <> TLSREC_LOCAL const LadderConsts<L256> &tlsks::ladder_consts<L256>() { return kConsts256; }
template <> TLSREC_LOCAL const LadderConsts<L384> &tlsks::ladder_consts<L384>() { return kConsts384; }

/* Host-only: the constants of `hash_alg` widened to 64 bits, zero_ip | zero_op |
 * d0_ip | d0_op | empty (40 words for SHA-256, 38 for SHA-384); returns the count. */
extern "C" int tlsrec__tls13_ladder_consts(int hash_alg, uint64_t *out)
{
    const int a = alg_index(hash_alg);
    if (a < 0 || !out) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return by_hash(a, [&](auto t) {
        typedef decltype(t) T;
        const LadderConsts<T> &k = ladder_consts<T>();
        int n = 0;
        for (int j = 0; j < 8; j++) out[n++] = k.zero_ip[j];
        for (int j = 0; j < 8; j++) out[n++] = k.zero_op[j];
        for (int j = 0; j < 8; j++) out[n++] = k.d0_ip[j];
        for (int j = 0; j < 8; j++) out[n++] = k.d0_op[j];
        for (int j = 0; j < T::HW; j++) out[n++] = k.empty[j];
        return n;
    });
}

static LadderLabels ladder_labels(size_t H, size_t key_len, const char *c_traffic, const char *s_traffic,
                                  const char *extra)
{
    LadderLabels lb;
    lb.derived = label_cells(H, "derived", 7, H);
    lb.c_traffic = label_cells(H, c_traffic, 12, H);
    lb.s_traffic = label_cells(H, s_traffic, 12, H);
    lb.extra = label_cells(H, extra, strlen(extra), H);
    lb.key = label_cells(key_len, "key", 3, 0);
    lb.iv = label_cells(12, "iv", 2, 0);
    lb.fin = label_cells(H, "finished", 8, 0);
    return lb;
}

/* the checks the two stages share, in the header's order; *alg: the suite's hash as in tlsrec_tls13_keytab_derive */
static int ladder_check(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, bool null_array, uint32_t psk_len,
                        uint32_t shared_len, int *alg)
{
    if (!kt || (null_array && count) || psk_len > 48) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!keytab_range_ok(kt, first, (uint64_t) count * 2)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (tlsrec_cipher_keylen(cipher) == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (shared_len != 0 && shared_len != 32 && shared_len != 48 && shared_len != 56 && shared_len != 66)
        return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    *alg = cipher == TLSREC_CIPHER_AES_256_GCM ? H_SHA384 : H_SHA256;
    return 0;
}

static uint32_t tls13_head(int cipher)
{
    /* tlsrec_key_material: cipher, tls_minor 4, fixed_ivlen 12 (ssl_tls13_keys.c:985-998), taglen */
    return (uint32_t) cipher | (4u << 8) | (12u << 16) | ((uint32_t) tlsrec_cipher_taglen(cipher) << 24);
}

template <class T>
static hipError_t hs_launch(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, uint32_t psk_len,
                            uint32_t shared_len, const tlsrec_tls13_hs_conn *conns, tlsrec_tls13_secret *hs_traffic,
                            tlsrec_tls13_secret *finished_keys, tlsrec_tls13_secret *master, hipStream_t st)
{
    Tls13HsArgs<T> a;
    a.conns = conns;
    a.out = tlsrec__keytab_stage(kt) + first;
    a.hs_traffic = hs_traffic;
    a.finished = finished_keys;
    a.master = master;
    a.count = count;
    a.head = tls13_head(cipher);
    a.key_cells = tlsrec_cipher_keylen(cipher) / 4;
    a.psk_len = psk_len;
    a.shared_len = shared_len;
    a.aligned = al(conns, AL_CONNS) | al(hs_traffic, AL_TRAFFIC) | al(finished_keys, AL_AUX) | al(master, AL_MASTER);
    a.k = ladder_consts<T>();
    a.lb = ladder_labels(T::HB, tlsrec_cipher_keylen(cipher), "c hs traffic", "s hs traffic", "");
    return launch_lanes(tls13_hs_kernel<T>, count, st, a);
}

/* The derive kernel alone (see tlsrec__tls13_stage_keys). */
extern "C" int tlsrec__tls13_stage_hs_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                           uint32_t psk_len, uint32_t shared_len, const tlsrec_tls13_hs_conn *conns,
                                           tlsrec_tls13_secret *hs_traffic, tlsrec_tls13_secret *finished_keys,
                                           tlsrec_tls13_secret *master, void *stream)
{
    int alg;
    int r = ladder_check(kt, first, count, cipher, !conns || !hs_traffic || !master, psk_len, shared_len, &alg);
    if (r != 0 || count == 0) return r;
    hipStream_t st = (hipStream_t) stream;
    return launch_status(by_hash(alg, [&](auto t) {
        return hs_launch<decltype(t)>(kt, first, count, cipher, psk_len, shared_len, conns, hs_traffic, finished_keys,
                                      master, st);
    }));
}

extern "C" int tlsrec_tls13_keytab_derive_handshake(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                                    uint32_t psk_len, uint32_t shared_len,
                                                    const tlsrec_tls13_hs_conn *conns, tlsrec_tls13_secret *hs_traffic,
                                                    tlsrec_tls13_secret *finished_keys, tlsrec_tls13_secret *master,
                                                    void *stream)
{
    int r = tlsrec__tls13_stage_hs_keys(kt, first, count, cipher, psk_len, shared_len, conns, hs_traffic, finished_keys,
                                        master, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, 2 * count, cipher, (hipStream_t) stream);
    return r;
}

template <class T>
static hipError_t app_launch(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                             const tlsrec_tls13_secret *master, const tlsrec_tls13_secret *transcripts,
                             tlsrec_tls13_secret *app_traffic, tlsrec_tls13_secret *exporter, hipStream_t st)
{
    Tls13AppArgs<T> a;
    a.master = master;
    a.transcripts = transcripts;
    a.out = tlsrec__keytab_stage(kt) + first;
    a.app_traffic = app_traffic;
    a.exporter = exporter;
    a.count = count;
    a.head = tls13_head(cipher);
    a.key_cells = tlsrec_cipher_keylen(cipher) / 4;
    a.aligned = al(master, AL_MASTER) | al(transcripts, AL_TRANSCRIPT) | al(app_traffic, AL_TRAFFIC) | al(exporter, AL_AUX);
    a.lb = ladder_labels(T::HB, tlsrec_cipher_keylen(cipher), "c ap traffic", "s ap traffic", "exp master");
    return launch_lanes(tls13_app_kernel<T>, count, st, a);
}

extern "C" int tlsrec__tls13_stage_app_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                            const tlsrec_tls13_secret *master, const tlsrec_tls13_secret *transcripts,
                                            tlsrec_tls13_secret *app_traffic, tlsrec_tls13_secret *exporter, void *stream)
{
    int alg;
    int r = ladder_check(kt, first, count, cipher, !master || !transcripts || !app_traffic, 0, 0, &alg);
    if (r != 0 || count == 0) return r;
    hipStream_t st = (hipStream_t) stream;
    return launch_status(by_hash(alg, [&](auto t) {
        return app_launch<decltype(t)>(kt, first, count, cipher, master, transcripts, app_traffic, exporter, st);
    }));
}

extern "C" int tlsrec_tls13_keytab_derive_application(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                                      const tlsrec_tls13_secret *master,
                                                      const tlsrec_tls13_secret *transcripts,
                                                      tlsrec_tls13_secret *app_traffic, tlsrec_tls13_secret *exporter,
                                                      void *stream)
{
    int r = tlsrec__tls13_stage_app_keys(kt, first, count, cipher, master, transcripts, app_traffic, exporter, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, 2 * count, cipher, (hipStream_t) stream);
    return r;
}

static int mac_launch(int hash_alg, uint32_t label_len, const unsigned char *label, const tlsrec_tls13_secret *keys,
                      const tlsrec_tls13_secret *msgs, tlsrec_tls13_secret *out, uint32_t count, void *stream)
{
    const int alg = alg_index(hash_alg);
    if (alg < 0) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if ((!keys || !msgs || !out) && count) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    if (!device_ready()) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls13MacArgs a;
    a.keys = keys;
    a.msgs = msgs;
    a.out = out;
    a.count = count;
    a.aligned = al(keys, AL_MASTER) | al(msgs, AL_TRANSCRIPT) | al(out, AL_AUX);
    a.label_len = label_len;
    memset(&a.label, 0, sizeof(a.label));
    if (label_len != MAC_PLAIN) a.label = label_cells(alg_len(alg), label, label_len, alg_len(alg));
    return launch_status(by_hash(alg, [&](auto t) {
        return launch_lanes(tls13_mac_kernel<decltype(t)>, count, (hipStream_t) stream, a);
    }));
}

extern "C" int tlsrec_tls13_batch_verify_data(int hash_alg, const tlsrec_tls13_secret *finished_keys,
                                              const tlsrec_tls13_secret *transcripts, tlsrec_tls13_secret *out,
                                              uint32_t count, void *stream)
{
    return mac_launch(hash_alg, MAC_PLAIN, nullptr, finished_keys, transcripts, out, count, stream);
}

extern "C" int tlsrec_tls13_batch_derive_secret(int hash_alg, const unsigned char *label, size_t label_len,
                                                const tlsrec_tls13_secret *secrets, const tlsrec_tls13_secret *transcripts,
                                                tlsrec_tls13_secret *out, uint32_t count, void *stream)
{
    if (label_len > 12 || (!label && label_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    return mac_launch(hash_alg, (uint32_t) label_len, label, secrets, transcripts, out, count, stream);
}

/* ---- a resumed handshake in batches (tls13_early_kernel, tls13_ticket_kernel) ---- */
/* the BAD_INPUT_DATA checks the binder and the early-key calls share, in the header's order */
static bool early_args_bad(bool null_array, uint32_t count, const void *offered, const void *binders, const void *match,
                           uint32_t psk_len)
{
    if (null_array && count) return true;
    if ((offered == nullptr) != (match == nullptr)) return true;
    if (!binders && !match && count) return true;
    return psk_len == 0 || psk_len > 48;
}

/* kt NULL: the binder alone, nothing staged */
template <class T>
static hipError_t early_launch(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher, uint32_t psk_len,
                               int psk_type, const tlsrec_tls13_psk_conn *conns, const tlsrec_tls13_secret *offered,
                               tlsrec_tls13_secret *binders, uint32_t *match, tlsrec_tls13_secret *early_traffic,
                               tlsrec_tls13_secret *early_exporter, hipStream_t st)
{
    Tls13EarlyArgs<T> a;
    a.conns = conns;
    a.offered = offered;
    a.binders = binders;
    a.match = match;
    a.out = kt ? tlsrec__keytab_stage(kt) + first : nullptr;
    a.early_traffic = early_traffic;
    a.early_exporter = early_exporter;
    a.count = count;
    a.head = kt ? tls13_head(cipher) : 0u;
    a.key_cells = kt ? tlsrec_cipher_keylen(cipher) / 4 : 0u;
    a.psk_len = psk_len;
    a.aligned = al(conns, AL_CONNS) | al(offered, AL_OFFERED) | al(binders, AL_BINDERS) | al(early_traffic, AL_TRAFFIC) |
                al(early_exporter, AL_AUX);
    a.k = ladder_consts<T>();
    /* ssl_tls13_keys.c:879-895: "res binder" for a resumption PSK, "ext binder" for any other type */
    a.binder = label_cells(T::HB, psk_type == TLSREC_TLS13_PSK_RESUMPTION ? "res binder" : "ext binder", 10, T::HB);
    a.c_e = label_cells(T::HB, "c e traffic", 11, T::HB);
    a.e_exp = label_cells(T::HB, "e exp master", 12, T::HB);
    memset(&a.lb, 0, sizeof(a.lb));
    a.lb.key = label_cells(kt ? tlsrec_cipher_keylen(cipher) : 0, "key", 3, 0);
    a.lb.iv = label_cells(12, "iv", 2, 0);
    a.lb.fin = label_cells(T::HB, "finished", 8, 0);
    return launch_lanes(tls13_early_kernel<T>, count, st, a);
}

extern "C" int tlsrec_tls13_batch_psk_binder(int hash_alg, uint32_t psk_len, int psk_type,
                                             const tlsrec_tls13_psk_conn *conns, const tlsrec_tls13_secret *offered,
                                             tlsrec_tls13_secret *binders, uint32_t *match, uint32_t count, void *stream)
{
    const int alg = alg_index(hash_alg);
    if (alg < 0 || early_args_bad(!conns, count, offered, binders, match, psk_len)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (count == 0) return 0;
    if (!device_ready()) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    return launch_status(by_hash(alg, [&](auto t) {
        return early_launch<decltype(t)>(nullptr, 0, count, 0, psk_len, psk_type, conns, offered, binders, match, nullptr,
                                         nullptr, (hipStream_t) stream);
    }));
}

/* The derive kernel alone (see tlsrec__tls13_stage_keys). */
extern "C" int tlsrec__tls13_stage_early_keys(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                              uint32_t psk_len, int psk_type, const tlsrec_tls13_psk_conn *conns,
                                              const tlsrec_tls13_secret *offered, tlsrec_tls13_secret *binders,
                                              uint32_t *match, tlsrec_tls13_secret *early_traffic,
                                              tlsrec_tls13_secret *early_exporter, void *stream)
{
    if (!kt || early_args_bad(!conns || !early_traffic, count, offered, binders, match, psk_len))
        return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!keytab_range_ok(kt, first, count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (tlsrec_cipher_keylen(cipher) == 0) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (count == 0) return 0;
    return launch_status(by_hash(cipher == TLSREC_CIPHER_AES_256_GCM ? H_SHA384 : H_SHA256, [&](auto t) {
        return early_launch<decltype(t)>(kt, first, count, cipher, psk_len, psk_type, conns, offered, binders, match,
                                         early_traffic, early_exporter, (hipStream_t) stream);
    }));
}

extern "C" int tlsrec_tls13_keytab_derive_early(tlsrec_keytab *kt, uint32_t first, uint32_t count, int cipher,
                                                uint32_t psk_len, int psk_type, const tlsrec_tls13_psk_conn *conns,
                                                const tlsrec_tls13_secret *offered, tlsrec_tls13_secret *binders,
                                                uint32_t *match, tlsrec_tls13_secret *early_traffic,
                                                tlsrec_tls13_secret *early_exporter, void *stream)
{
    int r = tlsrec__tls13_stage_early_keys(kt, first, count, cipher, psk_len, psk_type, conns, offered, binders, match,
                                           early_traffic, early_exporter, stream);
    if (r == 0 && count) r = tlsrec__keytab_commit_staged(kt, first, count, cipher, (hipStream_t) stream);
    return r;
}

extern "C" int tlsrec_tls13_batch_ticket_psk(int hash_alg, uint32_t nonce_len, const tlsrec_tls13_secret *res_master,
                                             const uint8_t *nonces, tlsrec_tls13_secret *psk, uint32_t count,
                                             void *stream)
{
    const int alg = alg_index(hash_alg);
    if (alg < 0 || ((!res_master || !nonces || !psk) && count)) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (nonce_len > 32) return TLSREC_ERR_SSL_FEATURE_UNAVAILABLE;
    if (count == 0) return 0;
    if (!device_ready()) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    Tls13TicketArgs a;
    a.res_master = res_master;
    a.nonces = nonces;
    a.psk = psk;
    a.count = count;
    a.aligned = al(res_master, AL_MASTER) | al(nonces, AL_TRANSCRIPT) | al(psk, AL_AUX);
    a.nonce_len = nonce_len;
    a.label = label_cells(alg_len(alg), "resumption", 10, nonce_len);
    return launch_status(by_hash(alg, [&](auto t) {
        return launch_lanes(tls13_ticket_kernel<decltype(t)>, count, (hipStream_t) stream, a);
    }));
}

