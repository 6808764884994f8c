/*
 * tlsrec_plan.h -- the launch shapes of a batch, as pure host functions.
 *
 * gcm_plan() and chacha_plan() decide, from a batch's record count, the key
 * table, the caller's hints and the TLSREC_GCM_* switches, which kernel family
 * runs and with what lanes per record, records per wave and grid.  Plain
 * C++17 without a HIP include: batch.hip launches what they return, a host
 * compiler can build and sweep them alone (tests/c/plan_sweep.cpp), and
 * tests/test_gcm_plan_cpu.py holds them to tests/golden/gcm_plan.json, the
 * shapes recorded on the device before the rule moved here.
 * stream_rx_plan() and dtls_rx_plan() do the same for stream.hip's receive
 * framing from the TLSREC_RX_* switches (tests/test_frame_plan_cpu.py).
 */
#ifndef TLSREC_PLAN_H
#define TLSREC_PLAN_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

namespace tlsrec {

constexpr int PLAN_GCM_WAVES = 16;   /* GCM_WAVES: waves of a key-pass workgroup (one workgroup per CU) */
constexpr int PLAN_CP_WAVES = 4;     /* CP_WAVES: waves of a ChaCha20-Poly1305 workgroup */

/* The TLSREC_GCM_* / TLSREC_GROUPED switches (measurement overrides and the
 * tests' second paths), with the values of an empty environment.  32-bit
 * fields only: mbedtls_amd/_abi.py mirrors the layout. */
struct GcmKnobs {
    int32_t waves = PLAN_GCM_WAVES;   /* _WAVES=8: 8 waves per key-pass workgroup (read once per process) */
    int32_t wp = -1;                  /* _WP: 1 forces the wave passes, 0 disables them, -1 (unset) = the rule */
    uint32_t g5 = 1;                  /* _G5=0: the 8-lane kernel's 4-bit GHASH Horner table instead of the 5-bit
                                         one (gmul5: 104 instead of 128 LDS cycles per multiply) */
    int32_t treemul = -1;             /* _TREEMUL: GcmArgs::tm bits 0..3 (gcm_tm below), -1 (unset) = per family */
    uint32_t hbuild = 1;              /* _HBUILD=0: the paired passes stage the Horner table from HBM (tm bit 4) */
    int32_t pair = 1;                 /* _PAIR=0: the 8-wave wave passes instead of the paired ones */
    uint32_t grouped = 1;             /* TLSREC_GROUPED=0: the stream / DTLS layers' batches go through the bucket
                                         pass as in r05 (BatchOpt::grouped; A/B and the tests' second path) */
    uint32_t srecs = 0;               /* _SRECS=1: key-ordered descriptor copy (bucket scatter).  Off: same box, k4
                                         665 vs 665-666, c4s 836 vs 840-843, c4 1032 vs 1035 GiB/s (profiles/r04h)
                                         -- the scattered 40-byte writes cost what the contiguous reads save */
    int32_t pair_l = 0;               /* _PAIR_L=2/4/8: lanes of the paired passes over small records, 0 = the model */
    uint32_t pair_small_min = 12;     /* _PAIR_SMALL_MIN (r04: 12), _PAIR_SMALL_MAX (r04: 128), _PAIR_BIG_MAX (r05: */
    uint32_t pair_small_max = 256;    /* 40; r04: 12): the records per key of the paired passes, below */
    uint32_t pair_big_max = 40;
    uint32_t lanes = 0;               /* _LANES: lanes per GCM record when the caller passes 0; 0 or unset = auto */
};

static inline int plan_env(const char *name, int unset)
{
    const char *e = getenv(name);
    return e ? atoi(e) : unset;
}

/* Once per batch() call: the tests flip the switches between calls. */
static inline GcmKnobs gcm_knobs_from_env(void)
{
    static const int waves = plan_env("TLSREC_GCM_WAVES", 0) == 8 ? 8 : PLAN_GCM_WAVES;
    GcmKnobs k;
    k.waves = waves;
    k.wp = plan_env("TLSREC_GCM_WP", -1);
    k.g5 = plan_env("TLSREC_GCM_G5", 1) != 0;
    const char *tm = getenv("TLSREC_GCM_TREEMUL");
    k.treemul = tm ? (atoi(tm) & 15) : -1;
    k.hbuild = plan_env("TLSREC_GCM_HBUILD", 1) != 0;
    k.pair = plan_env("TLSREC_GCM_PAIR", 1);
    k.grouped = plan_env("TLSREC_GROUPED", 1) != 0;
    k.srecs = plan_env("TLSREC_GCM_SRECS", 0) == 1;
    const int pl = plan_env("TLSREC_GCM_PAIR_L", 0);
    k.pair_l = (pl == 2 || pl == 4 || pl == 8) ? pl : 0;
    k.pair_small_min = (uint32_t) plan_env("TLSREC_GCM_PAIR_SMALL_MIN", 12);
    k.pair_small_max = (uint32_t) plan_env("TLSREC_GCM_PAIR_SMALL_MAX", 256);
    k.pair_big_max = (uint32_t) plan_env("TLSREC_GCM_PAIR_BIG_MAX", 40);
    k.lanes = (uint32_t) plan_env("TLSREC_GCM_LANES", 0);
    return k;
}

struct GcmPlanIn {
    uint32_t n;           /* records of the batch */
    uint32_t nloaded;     /* slots of the table holding a key */
    uint32_t cu;          /* compute units of the device */
    uint32_t avg_bytes;   /* mean record size when the caller knows it (stream / DTLS layers, host pipeline), else 0 */
    uint32_t lanes;       /* the caller's lanes per record, after the TLSREC_GCM_LANES fallback; 0 = auto */
    uint32_t nr;          /* AES rounds: 10 / 12 / 14 (AES-192 has key-pass kernels only) */
    uint32_t has_cid;     /* the table holds DTLS connection IDs: the CID variant, one configuration */
    uint32_t coalesced;   /* records gathered from concurrent single-record calls, each with its own key */
    uint32_t keyrun;      /* a key's records are found as a run (bucket pass, or already grouped): the many-keys
                             shapes apply */
};

struct GcmPlan {
    int32_t L;        /* lanes per record */
    int32_t waves;    /* waves per workgroup */
    int32_t code;     /* tlsrec__launch_gcm's waves argument and the launch log's: -32 paired wave passes, -8 wave
                         passes, -16 the CID variant, else waves */
    uint32_t rpw;     /* GcmArgs::rpw, ::tm, ::g5 */
    uint32_t tm;
    uint32_t g5;
    uint32_t grid;
};

struct ChachaPlan {
    int32_t L;
    uint32_t rpw, grid;
};

/* records per wave: the batch over target_wgs workgroups, in whole rounds of R records, at most 64 */
static inline uint32_t pick_rpw(uint64_t n, uint32_t waves_per_wg, uint32_t R, uint32_t target_wgs)
{
    const uint64_t per_round = (uint64_t) waves_per_wg * (target_wgs ? target_wgs : 1);
    uint64_t want = (n + per_round - 1) / per_round;
    if (want < R) want = R;
    want = (want + R - 1) / R * R;
    if (want > 64) want = 64;
    return (uint32_t) want;
}

static inline uint32_t plan_grid(uint64_t n, uint32_t waves, uint32_t rpw)
{
    const uint64_t per_wg = (uint64_t) waves * rpw;
    return (uint32_t) ((n + per_wg - 1) / per_wg);
}

/* a caller's lane request the GCM kernels have; anything else means auto */
static inline bool gcm_lanes_valid(uint32_t l) { return l == 2 || l == 4 || l == 8 || l == 16 || l == 64; }

/* Lanes per record of the paired passes over small records, from the mean
 * records per key (r05).  Each half of a pair takes about rpk / 2 of a key's
 * records in rounds of R = 64 / L records, so a key pass fills
 *     eff(L) = (rpk / 2) / (R * ceil(rpk / (2 R)))
 * of its rounds; the L with the best eff(L) x base(L) wins, base = the
 * full-round rates measured at 64 / 128 records per key (1 400-B AES-256-GCM,
 * 2 : 4 : 8 lanes = 603 : 590 : 530 GiB/s).  The model against the same-box
 * sweep (profiles/r05/small_rpk/), best measured lane count in brackets:
 *   rpk      16  23  32  47  64  95  128  191
 *   model     8   4   4   8   2   4    2    2
 *   [best]    8   4   4   8   2   4    2    2
 * r04's rule (2 from 48, 4 from 24, else 8) lost 14-29 % at 47 and 95 per
 * key, and the 16-wave key passes it used from 128 per key 13-25 %. */
static inline uint32_t gcm_pair_small_l(uint32_t rpk)
{
    static const uint32_t Ls[3] = { 2, 4, 8 };
    static const double base[3] = { 1.0, 590.0 / 603.0, 530.0 / 603.0 };
    double best = -1.0;
    uint32_t bl = 8;
    const double h = rpk / 2.0;
    for (int i = 0; i < 3; i++) {
        const double R = 64.0 / Ls[i];
        const double rounds = ceil(h / R);
        const double score = rounds > 0 ? base[i] * h / (R * rounds) : 0.0;
        if (score > best + 1e-9) {
            best = score;
            bl = Ls[i];
        }
    }
    return bl;
}

/* GcmArgs::tm, the table-free multiplies of the wave passes (tlsrec_clmul.h):
 *   bit 0  the 16-lane tree instead of the key's H^8 / H^4 / H^2 / H^1 tables
 *          from HBM (24 KiB more per key pass).  Default on.  Same box: k4
 *          455 -> 461 GiB/s, stream 4 x 16 KiB per key receive 424/429 -> 432/432
 *   bit 1  the 2- and 4-lane trees.  Default on for the paired passes (c4s
 *          740 -> 750 GiB/s same-box; +-1 % in the 8-wave passes)
 *   bit 2  the AAD fold and the two final multiplies by H as a value.  Default
 *          on for the paired passes (c4s 720 -> 742, k4 549 -> 558, 64 K keys x
 *          16 x 1.4 KiB 362 -> 377 GiB/s: the key's 8 KiB H^1 table in global
 *          memory cost 32 lines per multiply)
 *   bit 3  (r04) lane powers: AAD and the length block in the lane layout, one
 *          multiply by H^(d+1) per lane and a lane XOR replace the fold, the
 *          tree and the final multiplies.  Default on for the wave passes (k4
 *          582 -> 636 GiB/s, DTLS 16 x 1.4 KiB +17 %); compiled into the
 *          wave-pass kernels only (the 16-wave key passes' LDS-table tree is
 *          cheaper than a VALU multiply on an LDS-bound kernel, and the
 *          run-time flag alone cost c2 5 %, tlsrec_gcm.h)
 *   bit 4  (r05) the paired passes build the key's Horner table in LDS from
 *          H^L (tlsrec_gtab4_window) instead of staging its 8 KiB from HBM per
 *          key pass
 * TLSREC_GCM_TREEMUL sets bits 0..3, TLSREC_GCM_HBUILD=0 clears bit 4. */
static inline uint32_t gcm_tm(bool pair, bool wp, const GcmKnobs &k)
{
    uint32_t tm = k.treemul >= 0 ? (uint32_t) k.treemul : (pair ? 15u : (wp ? 9u : 1u));
    if (pair && k.hbuild) tm |= 16u;
    return tm;
}

static inline GcmPlan gcm_plan(const GcmPlanIn &in, const GcmKnobs &k)
{
    const uint32_t n = in.n, nl = in.nloaded, avg = in.avg_bytes;
    const uint64_t cu = in.cu ? in.cu : 1;
    const bool auto_l = !gcm_lanes_valid(in.lanes);
    const bool small_rec = avg != 0 && avg <= 4096;             /* the size hint says <= 4 KiB */
    const uint32_t rpk = nl > 1 ? n / nl : n;                   /* mean records per key */
    /* the wave-pass kernel families exist for AES-128 / -256 without CIDs, over runs of a key's records */
    const bool many = !in.has_cid && in.keyrun && in.nr != 12;

    /* Key passes (16 waves, the workgroup stages one key's tables): a key
     * pass should still fill the workgroup's 16 waves -- 8 lanes for a single
     * key or >= 128 records per key, 16 (4 records per wave) down to 48, 64
     * (one record per wave) below.  And the batch should fill the chip: with
     * fewer than 8 records per wave of a full grid (cu x 16 waves), more lanes
     * (16 K x 16 KiB records: L = 8 363, L = 16 611, L = 64 536 GiB/s). */
    const uint64_t rpwave = n / (cu * PLAN_GCM_WAVES);
    const int Lfill = rpwave >= 8 ? 8 : (rpwave >= 2 ? 16 : 64);
    int L = !auto_l ? (int) in.lanes : (nl <= 1 || rpk >= 128) ? 8 : (rpk >= 48 ? 16 : 64);
    if (auto_l && Lfill > L) L = Lfill;
    /* One key, small records: 4 lanes (16 records per wave round) once the
     * batch fills the chip at that -- half the lane tree and twice the records
     * in flight per wave.  Same box (r04r): c2s 592/582 -> 652/661, c2se
     * 610/604 -> 682/681 GiB/s; 16 KiB records keep 8 (c2 750/742 at 8,
     * 732/737 at 4). */
    if (auto_l && nl <= 1 && L == 8 && rpwave >= 16 && small_rec) L = 4;
    if (in.has_cid) L = 8;

    /* Wave passes (8 waves, each stages only its key's H^L table, no
     * workgroup barriers) for tables of many keys with little work each: under
     * 12 records per key, where a workgroup-wide key pass leaves most waves
     * idle, or -- the size known -- under 64 KiB per key (same box: 16 x
     * 1.4 KiB per key 198 -> 313 GiB/s, DTLS 125 -> 231; 16 x 16 KiB and 64 x
     * 1.4 KiB per key stay faster with key passes).  16 lanes (a wave's 4
     * records share one key pass) from 3 records per key, 64 below; 256 K x
     * 16 KiB AES-256-GCM decrypt (GiB/s):
     *   records/key        1     2     4     8    16    32
     *   wave passes L=16   90   177   415   423   429   433
     *   wave passes L=64  212   228   244   255   259   267
     *   workgroup passes   56   108   208   369   536   584
     * Small records, 12..127 per key: 4 lanes (16 of the key's records per
     * round) once the batch fills the chip at 16 per wave -- one lane tree per
     * 16 records, only H^1, H^2 read from HBM -- and 2 lanes (32 per round,
     * only H^1) from 48 per key.  Same box, 1.4 KiB records, from L = 16:
     *   64 K keys x 16, DTLS AES-128-GCM   receive 232 -> 390, send 212 -> 328 GiB/s
     *   64 K keys x 16, stream AES-256-GCM receive 198 -> 335, send 200 -> 294
     *   16 K keys x 64, stream AES-256-GCM receive 317 -> 357, send 282 -> 324
     *   c4s (64 K keys x 64, GCM + ChaCha)  486 -> 541
     *   2 lanes: 16 K keys x 64 receive 353 -> 375, send 319 -> 332, c4s 536 ->
     *   549 (at 16 per key 2 lanes idle half the wave: 388 -> 254). */
    const bool small = small_rec && rpk >= 12 && rpk < 128;
    const bool small2 = small && rpk >= 48 && n >= cu * 8 * 32;
    const bool small4 = small && !small2 && n >= cu * 8 * 16;
    const bool light = rpk < 12 || (avg != 0 && rpk < 48 && (uint64_t) rpk * avg < 65536u) || small2 || small4;
    if (auto_l && many && k.wp != 0 && light) L = small2 ? 2 : (small4 ? 4 : ((rpk >= 3 && Lfill <= 16) ? 16 : 64));
    bool wp = many && (L == 2 || L == 4 || L == 16 || L == 64) && (k.wp == 1 || (k.wp != 0 && light));
    /* coalesced: a wave per record, 64 lanes on it -- each wave its own record's key, in parallel */
    if (in.coalesced && n > 1 && auto_l && !in.has_cid && in.nr != 12) {
        L = 64;
        wp = true;
    }

    /* Paired wave passes (16 waves, two per key table).  The 8-wave passes
     * hold one 8 KiB H^L table per wave beside the 64 KiB T-tables, so they
     * run at half the single-key kernel's occupancy and wait on LDS latency
     * (r02 PMC, DTLS 16 x 1.4 KiB per key: LDS 35 %, VALU 53 % busy); with two
     * waves per table, 16 waves fit.  Small records, 12..255 per key (r05;
     * from 128 the key passes lost 13-25 %): each wave takes half of a key's
     * records, L by the round-fill model above.  Large records (known >
     * 4 KiB), 4..39 per key (k4, 16 KiB streams): 32 lanes below 8 per key, 16
     * from there.  With the rounds starting at each key's first position
     * (tlsrec_gcm.h), 16 KiB records, 2^18 records (same box,
     * profiles/r05/pair_big), 16-wave key passes -> paired 16 lanes:
     *   records per key     16          23          32          47
     *   GiB/s            637 -> 705  638 -> 667  667 -> 711  668 -> 654
     * and the stream layer's 64 K connections x 16 x 16 KiB receive / send
     * 602 -> 685 / 497 -> 542; at 64 per key one key fills a key pass's 16
     * waves exactly and the key passes stay (c4).  The batch must fill the
     * chip's 16 waves per CU at 64 / L records each.  (r06) the paired kernels
     * hold lane powers only (tlsrec_gcm.h): a coalesced call or a TREEMUL mode
     * without bit 3 takes the 8-wave passes. */
    bool pair = false;
    if (auto_l && many && k.wp != 0 && k.pair && avg != 0 && !in.coalesced && (gcm_tm(true, true, k) & 8u)) {
        int Lp = 0;
        const bool small_pair = avg <= 4096 && rpk >= k.pair_small_min && rpk < k.pair_small_max;
        if (small_pair) Lp = k.pair_l ? k.pair_l : (int) gcm_pair_small_l(rpk);
        else if (avg > 4096 && rpk >= 4 && rpk < k.pair_big_max) Lp = rpk >= 8 ? 16 : 32;
        if (Lp && n >= cu * 16 * (uint64_t) (64 / Lp)) {
            L = Lp;
            wp = pair = true;
        }
    }
    if (L == 2 && !wp) L = 4;     /* 2 lanes: wave passes only */

    GcmPlan p;
    p.L = L;
    p.waves = pair ? 16 : (wp ? 8 : (in.has_cid ? 16 : k.waves));
    p.code = pair ? -32 : (wp ? -8 : (in.has_cid ? -16 : p.waves));
    p.rpw = (in.coalesced && wp) ? 1u : pick_rpw(n, (uint32_t) p.waves, 64u / (uint32_t) L, (uint32_t) cu);
    p.g5 = k.g5;
    /* coalesced calls wait on the lane tree: from the key's tables (one L2
     * round trip per level) rather than table-free (~1 700 dependent VALU
     * ticks per level) */
    p.tm = in.coalesced ? 0u : gcm_tm(pair, wp, k);
    p.grid = plan_grid(n, (uint32_t) p.waves, p.rpw);
    return p;
}

/* ChaCha20-Poly1305: 2 lanes per record, more when the batch would not fill
 * the chip (cu x 8 resident waves: 2 per SIMD); lanes_in is the caller's own
 * request (1 / 2 / 4 / 8, else auto); the CID variant is one configuration */
static inline ChachaPlan chacha_plan(uint32_t n, uint32_t cu, uint32_t lanes_in, bool has_cid)
{
    if (cu == 0) cu = 1;
    const uint64_t rpwave = (uint64_t) n / ((uint64_t) cu * 8);
    ChachaPlan p;
    p.L = (lanes_in == 1 || lanes_in == 2 || lanes_in == 4 || lanes_in == 8) ? (int) lanes_in
          : (rpwave >= 32 ? 2 : (rpwave >= 16 ? 4 : 8));
    if (has_cid) p.L = 2;
    p.rpw = pick_rpw(n, PLAN_CP_WAVES, 64u / (uint32_t) p.L, cu * 4);
    p.grid = plan_grid(n, PLAN_CP_WAVES, p.rpw);
    return p;
}

/* ---- receive framing (stream.hip) -------------------------------------- */
constexpr uint32_t PLAN_RX_THREADS = 256;   /* RX_THREADS: a stream count / emit workgroup, 256 / G connections */
constexpr uint32_t PLAN_RX_TILE = 128;      /* connections of a one-pass stream tile, at every G (in_frame_kernel) */
constexpr uint32_t PLAN_DG_TILE = 256;      /* DG_THREADS: connections of a DTLS tile, one lane each */

/* The switches of the stream / DTLS layers and their values in an empty environment: the default path against a
 * second one kept for A/B runs and tests.  32-bit fields only: mbedtls_amd/_abi.py mirrors the layout. */
struct FrameKnobs {
    uint32_t groupwalk = 1;      /* TLSREC_RX_GROUPWALK=0: one lane per connection (G = 1), never one pass */
    uint32_t fused_stream = 0;   /* TLSREC_RX_FUSED_STREAM=1: stream receive framing in one pass */
    int32_t rg = 0;              /* TLSREC_RX_RG=4|8|16: forces the lanes per connection; anything else = the rule */
    uint32_t fused = 1;          /* TLSREC_RX_FUSED=0: DTLS receive framing as count, scan and emit kernels */
    uint32_t stash = 1;          /* TLSREC_DTLS_STASH=0: the DTLS one pass without its LDS header copy */
    uint32_t prefill = 1;        /* TLSREC_RX_PREFILL=0: the receive batch runs its guard kernel */
    uint32_t mailbox = 1;        /* TLSREC_RX_MAILBOX=0: the totals by copies and a stream synchronize */
    uint32_t stream_src = 1;     /* TLSREC_STREAM_SRC=0: the send paths copy the application data first */
};

static inline FrameKnobs frame_knobs_from_env(void)   /* once per call: the tests flip the switches between calls */
{
    return { plan_env("TLSREC_RX_GROUPWALK", 1) != 0, plan_env("TLSREC_RX_FUSED_STREAM", 0) != 0,
             plan_env("TLSREC_RX_RG", 0), plan_env("TLSREC_RX_FUSED", 1) != 0, plan_env("TLSREC_DTLS_STASH", 1) != 0,
             plan_env("TLSREC_RX_PREFILL", 1) != 0, plan_env("TLSREC_RX_MAILBOX", 1) != 0,
             plan_env("TLSREC_STREAM_SRC", 1) != 0 };
}

static inline uint32_t plan_blocks(uint64_t n, uint32_t per) { return (uint32_t) ((n + per - 1) / per); }

struct StreamRxPlan {
    uint32_t fused;        /* count, scan and emit in one pass (the launch log's p0) */
    int32_t G;             /* lanes per connection: 1 / 4 / 8 / 16 (the launch log's p1) */
    uint32_t tile, tiles;             /* one pass: connections per tile, and the tiles = its grid */
    uint32_t count_grid, emit_grid;   /* else: workgroups of 256 / G connections over nstreams + 1 (sentinel), nstreams */
};

/* Stream receive.  Lanes per connection: the records a connection holds on average by the caller's capacity
 * (max_records / connections) -- 4, 8 or 16 (r06: a 4-record stream left 12 of 16 lanes idle) */
static inline StreamRxPlan stream_rx_plan(uint32_t nstreams, uint32_t max_records, const FrameKnobs &k)
{
    const uint64_t per = nstreams ? ((uint64_t) max_records + nstreams - 1) / nstreams : 16;
    const int32_t g = !k.groupwalk ? 1 : (k.rg == 4 || k.rg == 8 || k.rg == 16) ? k.rg : per <= 4 ? 4 : (per <= 8 ? 8 : 16);
    const uint32_t conns = PLAN_RX_THREADS / (uint32_t) g;
    return { k.fused_stream && k.groupwalk, g, PLAN_RX_TILE, plan_blocks(nstreams, PLAN_RX_TILE),
             plan_blocks((uint64_t) nstreams + 1, conns), plan_blocks(nstreams, conns) };
}

struct DtlsRxPlan {
    uint32_t fused;   /* count, scan and emit in one pass */
    int32_t S;        /* its LDS stash depth: 4 / 16 / 0 records per connection; -1 = three kernels (the log's p0) */
    uint32_t tiles;   /* tiles of PLAN_DG_TILE connections = the one pass's grid */
};

/* DTLS receive.  The one pass keeps LDS for a mean connection's records (4 / 16: 24 / 96 KiB per workgroup);
 * beyond 16 datagrams per connection, or with TLSREC_DTLS_STASH=0, its emit walks the headers again. */
static inline DtlsRxPlan dtls_rx_plan(uint32_t nconns, uint32_t ndgrams, const FrameKnobs &k)
{
    const uint64_t per = nconns ? ((uint64_t) ndgrams + nconns - 1) / nconns : 0;
    const int32_t s = !k.fused ? -1 : (!k.stash || per > 16) ? 0 : (per > 4 ? 16 : 4);
    return { k.fused != 0, s, plan_blocks(nconns, PLAN_DG_TILE) };
}

} /* namespace tlsrec */

#endif
