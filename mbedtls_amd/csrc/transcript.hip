/*
 * transcript.hip -- running handshake hashes on the GPU, in batches
 * (tlsrec_transcript_batch_update).
 *
 *   reference                                                here
 *   update_checksum                      ssl_tls.c:896-915   absorb() over a segment's bytes
 *   mbedtls_ssl_reset_checksum           ssl_tls.c:838       TLSREC_TRANSCRIPT_RESET
 *   mbedtls_ssl_get_handshake_transcript ssl_tls.c:5877-5925 digest() on a copy of the state
 *   mbedtls_ssl_reset_transcript_for_hrr
 *                        ssl_tls13_generic.c:1399-1441       TLSREC_TRANSCRIPT_HRR
 *
 * One connection per lane, 64 lanes per workgroup, no LDS, on sha_compress<T>
 * of tlsrec_sha.h like the ladders of tls13_ladder.hip.  A lane loads its state
 * (chaining words, byte count, partial block), walks its segments and stores
 * the state back.  The message window is 16 words in registers, addressed in
 * 32-bit big-endian cells (16 to a SHA-256 block, 32 to a SHA-512 one).
 *
 * A segment starts at any byte and meets a block at any fill level, so source
 * and block are out of phase in general.  With q = (address of the next source
 * byte) - fill, the place where byte 0 of the block would lie, cell c is the 4
 * bytes at q + 4c: they come from the two aligned source words around them,
 * joined and byte-swapped by one v_perm_b32 whose selector depends only on
 * q & 3.  Whole blocks take that path with unchecked aligned loads (16-byte
 * ones when q is 16-byte aligned), issued one block ahead of the compression
 * that hides them; a block that touches either end of its segment takes the
 * same path with every load checked against the segment, a word at a time
 * and by bytes for a word that straddles an end.  No byte outside
 * [off, off + len) of a segment is ever read.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tlsrec.h"
#include "tlsrec_sha.h"

namespace tlsks {

static_assert(sizeof(tlsrec_transcript_state) == 208 && offsetof(tlsrec_transcript_state, count) == 64 &&
              offsetof(tlsrec_transcript_state, hash) == 72 && offsetof(tlsrec_transcript_state, block) == 80,
              "tlsrec_transcript_state layout");
static_assert(sizeof(tlsrec_transcript_seg) == 24 && sizeof(tlsrec_transcript_conn) == 16, "transcript item layouts");

/* the shapes of one hash, from its compression's word type */
template <class T> struct TrShape {
    typedef typename T::W W;
    static constexpr uint32_t BB = 16 * sizeof(W);       /* block bytes */
    static constexpr uint32_t NC = BB / 4;               /* cells per block */
    static constexpr uint32_t HB = sizeof(W) == 4 ? 32 : 48;   /* Hash.length */
    static constexpr uint32_t LENB = 2 * sizeof(W);      /* bytes of the length field */
    static constexpr uint32_t ID = sizeof(W) == 4 ? TLSREC_ALG_SHA_256 : TLSREC_ALG_SHA_384;
};

/* cell c of a block or digest; c is a constant wherever these are used */
template <class W, int N> __device__ __forceinline__ void tr_or_cell(W (&w)[N], int c, uint32_t v)
{
    if constexpr (sizeof(W) == 4) w[c] |= v;
    else w[c >> 1] |= (uint64_t) v << ((c & 1) ? 0 : 32);
}
template <class W, int N> __device__ __forceinline__ uint32_t tr_cell(const W (&w)[N], int c)
{
    if constexpr (sizeof(W) == 4) return w[c];
    else return (c & 1) ? (uint32_t) w[c >> 1] : (uint32_t) (w[c >> 1] >> 32);
}

__device__ __forceinline__ uint32_t tr_ld32(uint64_t a) { return *reinterpret_cast<const uint32_t *>((uintptr_t) a); }
__device__ __forceinline__ uint32_t tr_ld8(uint64_t a) { return *reinterpret_cast<const uint8_t *>((uintptr_t) a); }

/* the aligned word at `a` as far as it lies in [lo, hi): bytes outside read as 0 and are not touched */
__device__ __forceinline__ uint32_t tr_load_chk(uint64_t a, uint64_t lo, uint64_t hi)
{
#ifndef TLSREC_TRANSCRIPT_BYTEWISE
    if (a >= lo && a + 4 <= hi) return tr_ld32(a);
#endif
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (a + b >= lo && a + b < hi) r |= tr_ld8(a + b) << (8 * b);
    return r;
}

/* big-endian cell from the memory bytes ph .. ph + 3 of the aligned word pair (x0 below x1):
 * v_perm_b32 takes bytes 0-3 from its second operand and 4-7 from its first */
__device__ __forceinline__ uint32_t tr_sel(uint32_t ph) { return 0x00010203u + ph * 0x01010101u; }
__device__ __forceinline__ uint32_t tr_join(uint32_t x0, uint32_t x1, uint32_t sel)
{
    return __builtin_amdgcn_perm(x1, x0, sel);
}

struct TranscriptArgs {
    tlsrec_transcript_state *states;
    const tlsrec_transcript_conn *conns;
    const tlsrec_transcript_seg *segs;
    const uint8_t *arena;
    uint8_t *out;
    int32_t *status;
    uint64_t arena_len, out_len;
    uint32_t nstates, nconns, nsegs;
};

__global__ void __launch_bounds__(64) transcript_prefill_kernel(int32_t *status, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) status[i] = TLSREC_ERR_SSL_INTERNAL_ERROR;
}

template <class T> __global__ void __launch_bounds__(64) transcript_kernel(TranscriptArgs a)
{
    typedef typename T::W W;
    typedef TrShape<T> SH;
    constexpr uint32_t BB = SH::BB, NC = SH::NC, HB = SH::HB;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nconns) return;
    const tlsrec_transcript_conn cn = a.conns[i];

    /* ---- every rule of the connection before its first byte ---- */
    bool bad = cn.state >= a.nstates || cn.reserved != 0 || (uint64_t) cn.first_seg + cn.nseg > a.nsegs;
    if (!bad) {
        for (uint32_t s = 0; s < cn.nseg; s++) {
            const tlsrec_transcript_seg sg = a.segs[cn.first_seg + s];
            if (sg.flags & ~(TLSREC_TRANSCRIPT_RESET | TLSREC_TRANSCRIPT_SNAPSHOT | TLSREC_TRANSCRIPT_HRR)) bad = true;
            if (sg.off > a.arena_len || sg.len > a.arena_len - sg.off) bad = true;
            if ((sg.flags & TLSREC_TRANSCRIPT_SNAPSHOT) && (a.out_len < 48 || sg.out_off > a.out_len - 48)) bad = true;
            /* only the first segment can meet a state of another hash: after it the state is this call's */
            if (s == 0 && !(sg.flags & TLSREC_TRANSCRIPT_RESET) && a.states[cn.state].hash != SH::ID) bad = true;
        }
    }
    if (bad) {
        a.status[i] = TLSREC_ERR_SSL_BAD_INPUT_DATA;
        return;
    }
    if (cn.nseg == 0) {
        a.status[i] = 0;
        return;
    }

    /* ---- the state: 26 8-byte words ---- */
    uint64_t *sp = reinterpret_cast<uint64_t *>(a.states + cn.state);
    W st[8], w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = (W) sp[j];
    uint64_t count = sp[8];
    uint32_t fill = (uint32_t) count & (BB - 1);
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
    for (uint32_t k = 0; k < NC / 2; k++) {
        const uint64_t v = sp[10 + k];
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            /* bytes at and past the fill level count as zero whatever the state holds there */
            const uint32_t c = 2 * k + h;
            const int keep = (int) fill - (int) (4 * c);
            const uint32_t mask = keep >= 4 ? 0xffffffffu : keep <= 0 ? 0u : 0xffffffffu << (8 * (4 - keep));
            tr_or_cell(w, c, __builtin_bswap32((uint32_t) (v >> (32 * h))) & mask);
        }
    }

    for (uint32_t s = 0; s < cn.nseg; s++) {
        const tlsrec_transcript_seg sg = a.segs[cn.first_seg + s];
        if (sg.flags & TLSREC_TRANSCRIPT_RESET) {
#pragma unroll
            for (int j = 0; j < 8; j++) st[j] = T::iv(j);
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = 0;
            count = 0;
            fill = 0;
        }

        /* ---- absorb [pos, end) ---- */
        const uint64_t p = (uint64_t) (uintptr_t) a.arena + sg.off, end = p + sg.len;
        uint64_t pos = p;
        uint32_t nx[NC + 1];        /* the next block's source words, loaded ahead of the compression */
#pragma unroll
        for (uint32_t c = 0; c <= NC; c++) nx[c] = 0;
        /* a whole block whose words (the one past it included when out of phase) lie inside the segment */
        auto whole = [&](uint64_t at) {
#ifdef TLSREC_TRANSCRIPT_BYTEWISE
            return false;
#else
            const uint32_t ph = (uint32_t) at & 3;
            return at - p >= ph && end - at >= BB + (ph ? 4u : 0u);
#endif
        };
        auto fetch = [&](uint64_t at) {
            const uint64_t a0 = at & ~(uint64_t) 3;
            if ((a0 & 15) == 0) {
#pragma unroll
                for (uint32_t c = 0; c < NC; c += 4) {
                    const uint4 v = *reinterpret_cast<const uint4 *>((uintptr_t) (a0 + 4 * c));
                    nx[c] = v.x; nx[c + 1] = v.y; nx[c + 2] = v.z; nx[c + 3] = v.w;
                }
            } else {
#pragma unroll
                for (uint32_t c = 0; c < NC; c++) nx[c] = tr_ld32(a0 + 4 * c);
            }
            nx[NC] = (at & 3) ? tr_ld32(a0 + BB) : 0u;
        };
        bool fast = fill == 0 && pos < end && whole(pos);
        if (fast) fetch(pos);
        while (pos < end) {
            bool full;
            if (fast) {
                const uint32_t sel = tr_sel((uint32_t) pos & 3);
#pragma unroll
                for (uint32_t c = 0; c < NC; c++) tr_or_cell(w, c, tr_join(nx[c], nx[c + 1], sel));
                pos += BB;
                count += BB;
                full = true;
            } else {
                /* up to the end of the block or of the segment, every load checked against [pos, pos + n) */
                const uint64_t left = end - pos;
                const uint32_t n = left < BB - fill ? (uint32_t) left : BB - fill;
                const uint64_t q = pos - fill, a0 = q & ~(uint64_t) 3, hi = pos + n;
                const uint32_t sel = tr_sel((uint32_t) q & 3);
                uint32_t x0 = tr_load_chk(a0, pos, hi);
#pragma unroll
                for (uint32_t c = 0; c < NC; c++) {
                    const uint32_t x1 = tr_load_chk(a0 + 4 * (c + 1), pos, hi);
                    tr_or_cell(w, c, tr_join(x0, x1, sel));
                    x0 = x1;
                }
                pos += n;
                count += n;
                fill += n;
                full = fill == BB;
            }
            fast = full && pos < end && whole(pos);
            if (fast) fetch(pos);
            if (full) {
                sha_compress<T>(st, w);
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = 0;
                fill = 0;
            }
        }

        /* ---- digest of a copy: the live state goes on ---- */
        if (sg.flags & (TLSREC_TRANSCRIPT_SNAPSHOT | TLSREC_TRANSCRIPT_HRR)) {
            W d[8], pw[16];
#pragma unroll
            for (int j = 0; j < 8; j++) d[j] = st[j];
#pragma unroll
            for (int j = 0; j < 16; j++) pw[j] = w[j];
#pragma unroll
            for (uint32_t c = 0; c < NC; c++)
                tr_or_cell(pw, c, c == (fill >> 2) ? 0x80000000u >> (8 * (fill & 3)) : 0u);
            /* the length does not fit behind a fill level of 56 / 112 and up: a second block */
#pragma unroll 1
            for (int k = fill >= BB - SH::LENB ? 0 : 1; k < 2; k++) {
                if (k == 1) {
                    if constexpr (sizeof(W) == 4) {
                        pw[14] |= (uint32_t) (count >> 29);
                        pw[15] |= (uint32_t) (count << 3);
                    } else {
                        pw[14] |= count >> 61;
                        pw[15] |= count << 3;
                    }
                }
                sha_compress<T>(d, pw);
#pragma unroll
                for (int j = 0; j < 16; j++) pw[j] = 0;
            }
            if (sg.flags & TLSREC_TRANSCRIPT_SNAPSHOT) {
                /* Hash.length bytes, then zeros up to 48 */
                uint32_t o[12];
#pragma unroll
                for (uint32_t c = 0; c < 12; c++) o[c] = c < HB / 4 ? __builtin_bswap32(tr_cell(d, c)) : 0u;
                uint8_t *dst = a.out + sg.out_off;
                if (((uintptr_t) dst & 15) == 0) {
                    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
#pragma unroll
                    for (int k = 0; k < 3; k++) d4[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
                } else {
#pragma unroll
                    for (uint32_t c = 0; c < 12; c++) {
#pragma unroll
                        for (int b = 0; b < 4; b++) dst[4 * c + b] = (uint8_t) (o[c] >> (8 * b));
                    }
                }
            }
            if (sg.flags & TLSREC_TRANSCRIPT_HRR) {
                /* a fresh hash that has absorbed message_hash: FE 00 00 Hash.length || digest, below one block */
#pragma unroll
                for (int j = 0; j < 8; j++) st[j] = T::iv(j);
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = 0;
                tr_or_cell(w, 0, 0xfe000000u | HB);
#pragma unroll
                for (uint32_t c = 0; c < HB / 4; c++) tr_or_cell(w, 1 + c, tr_cell(d, c));
                count = 4 + HB;
                fill = 4 + HB;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) d[j] = 0;
        }
    }

    /* ---- the state back ---- */
#pragma unroll
    for (int j = 0; j < 8; j++) sp[j] = (uint64_t) st[j];
    sp[8] = count;
    sp[9] = SH::ID;          /* hash, reserved = 0 */
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        uint64_t v = 0;
        if (2 * k < NC)
            v = (uint64_t) __builtin_bswap32(tr_cell(w, 2 * k)) | ((uint64_t) __builtin_bswap32(tr_cell(w, 2 * k + 1)) << 32);
        sp[10 + k] = v;
    }
    a.status[i] = 0;
}

}  // namespace tlsks

using namespace tlsks;

extern "C" int tlsrec_transcript_batch_update(int hash_alg, tlsrec_transcript_state *states, uint32_t nstates,
                                              const tlsrec_transcript_conn *conns, uint32_t nconns,
                                              const tlsrec_transcript_seg *segs, uint32_t nsegs,
                                              const uint8_t *arena, uint64_t arena_len, uint8_t *out_arena,
                                              uint64_t out_len, int32_t *status, void *stream)
{
    if (hash_alg != TLSREC_ALG_SHA_256 && hash_alg != TLSREC_ALG_SHA_384) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if ((!states || !conns || !status) && nconns) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!segs && nsegs) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!arena && arena_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (!out_arena && out_len) return TLSREC_ERR_SSL_BAD_INPUT_DATA;
    if (nconns == 0) return 0;
    static const int device = tlsrec_device_check();     /* no key table vouches for a device here; asked once */
    if (device != 0) return TLSREC_ERR_SSL_HW_ACCEL_FAILED;
    TranscriptArgs a;
    a.states = states;
    a.conns = conns;
    a.segs = segs;
    a.arena = arena;
    a.out = out_arena;
    a.status = status;
    a.arena_len = arena_len;
    a.out_len = out_len;
    a.nstates = nstates;
    a.nconns = nconns;
    a.nsegs = nsegs;
    hipStream_t st = (hipStream_t) stream;
    const dim3 grid((nconns + 63) / 64), block(64);
    /* fail closed: every status reads INTERNAL_ERROR until the kernel has decided it */
    hipLaunchKernelGGL(transcript_prefill_kernel, grid, block, 0, st, status, nconns);
    if (hash_alg == TLSREC_ALG_SHA_384) hipLaunchKernelGGL(transcript_kernel<S512>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(transcript_kernel<S256>, grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : TLSREC_ERR_SSL_HW_ACCEL_FAILED;
}
