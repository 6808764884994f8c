/*
 * plan_sweep -- sweeps gcm_plan() and chacha_plan() (mbedtls_amd/csrc/tlsrec_plan.h)
 * over record counts, key counts, size hints, CU counts and lane requests far
 * outside what a device run can reach, under -fsanitize=address,undefined
 * (tests/c/Makefile plan_sweep): no division by zero or overflow, a lane count
 * the kernels have, a grid that covers the batch; and stream_rx_plan() /
 * dtls_rx_plan() over connection, record and datagram counts up to 2^32 - 1.
 * Host only: no library, no device.  Exit status 0 = every plan held.
 */
#include <stdio.h>

#include "tlsrec_plan.h"

using namespace tlsrec;

static int fails = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond) && fails++ < 20) {        \
            fprintf(stderr, "%s: ", #cond);   \
            fprintf(stderr, __VA_ARGS__);     \
            fputc('\n', stderr);              \
        }                                     \
    } while (0)

static void check_gcm(const GcmPlanIn &in, const GcmKnobs &k)
{
    const GcmPlan p = gcm_plan(in, k);
    const bool known = p.L == 2 || p.L == 4 || p.L == 8 || p.L == 16 || p.L == 32 || p.L == 64;
    CHECK(known, "L=%d n=%u nloaded=%u cu=%u avg=%u lanes=%u", p.L, in.n, in.nloaded, in.cu, in.avg_bytes, in.lanes);
    if (!known) return;
    CHECK(p.waves == 8 || p.waves == 16, "waves=%d", p.waves);
    CHECK(p.rpw >= 1 && p.rpw <= 64, "rpw=%u", p.rpw);
    CHECK(p.rpw == 1 || p.rpw % (64u / (uint32_t) p.L) == 0, "rpw=%u L=%d", p.rpw, p.L);
    if (in.n == 0) return;       /* batch() launches nothing; the plan only must not trap */
    const uint64_t per_wg = (uint64_t) p.waves * p.rpw;
    CHECK(p.grid >= 1, "grid=%u n=%u", p.grid, in.n);
    CHECK(p.grid * per_wg >= in.n && (p.grid - 1) * per_wg < in.n, "grid=%u per_wg=%llu n=%u", p.grid,
          (unsigned long long) per_wg, in.n);
}

int main(void)
{
    uint32_t ns[20] = { 0, 1, 2, 63, 64, 65 };
    int nn = 6;
    for (int s = 10; s <= 22; s++) ns[nn++] = 1u << s;
    static const uint32_t nls[] = { 0, 1, 2, 1u << 16, 1u << 20 };
    static const uint32_t avgs[] = { 0, 1, 4096, 4097, 1u << 24 };
    static const uint32_t cus[] = { 0, 1, 256 };
    static const uint32_t lanes[] = { 0, 1, 2, 3, 4, 8, 16, 32, 64, 0xffffffffu };
    static const uint32_t nrs[] = { 10, 12, 14 };
    GcmKnobs knobs[6];
    knobs[1].wp = 1;
    knobs[2].wp = 0;
    knobs[3].pair = 0;
    knobs[4].treemul = 7;
    knobs[4].waves = 8;
    knobs[5].pair_l = 2;
    knobs[5].pair_small_min = 0;
    knobs[5].pair_small_max = 0xffffffffu;
    knobs[5].pair_big_max = 0xffffffffu;
    long plans = 0;
    for (int a = 0; a < nn; a++)
        for (uint32_t nl : nls)
            for (uint32_t avg : avgs)
                for (uint32_t cu : cus)
                    for (uint32_t l : lanes) {
                        for (uint32_t nr : nrs)
                            for (uint32_t flags = 0; flags < 8; flags++)
                                for (const GcmKnobs &k : knobs) {
                                    const GcmPlanIn in = { ns[a], nl, cu, avg, l, nr, flags & 1, (flags >> 1) & 1,
                                                           (flags >> 2) & 1 };
                                    check_gcm(in, k);
                                    plans++;
                                }
                        for (int cid = 0; cid < 2; cid++) {
                            const ChachaPlan p = chacha_plan(ns[a], cu, l, cid != 0);
                            CHECK(p.L == 1 || p.L == 2 || p.L == 4 || p.L == 8, "chacha L=%d", p.L);
                            CHECK(p.rpw >= 1 && p.rpw <= 64 && p.rpw % (64u / (uint32_t) p.L) == 0, "chacha rpw=%u", p.rpw);
                            const uint64_t per_wg = (uint64_t) PLAN_CP_WAVES * p.rpw;
                            if (ns[a])
                                CHECK(p.grid >= 1 && p.grid * per_wg >= ns[a] && (p.grid - 1) * per_wg < ns[a],
                                      "chacha grid=%u n=%u", p.grid, ns[a]);
                            plans++;
                        }
                    }
    /* the lane model itself, every records-per-key count a uint32 division can give */
    for (uint32_t rpk = 0; rpk < (1u << 20); rpk += (rpk < 4096 ? 1 : 997)) {
        const uint32_t l = gcm_pair_small_l(rpk);
        CHECK(l == 2 || l == 4 || l == 8, "pair_small_l(%u)=%u", rpk, l);
    }
    /* the receive framing plans: every switch value, counts up to 2^32 - 1 */
    static const uint32_t cs[] = { 0, 1, 2, 127, 128, 129, 255, 256, 257, 1u << 16, 0x7fffffffu, 0xffffffffu };
    static const int32_t rgs[] = { 0, 1, 4, 5, 8, 16, -1, 0x7fffffff };
    for (uint32_t n : cs)
        for (uint32_t m : cs)
            for (uint32_t sw = 0; sw < 16; sw++)
                for (int32_t rg : rgs) {
                    FrameKnobs k;
                    k.groupwalk = sw & 1;
                    k.fused_stream = (sw >> 1) & 1;
                    k.fused = (sw >> 2) & 1;
                    k.stash = (sw >> 3) & 1;
                    k.rg = rg;
                    const StreamRxPlan p = stream_rx_plan(n, m, k);
                    CHECK(p.G == 1 || p.G == 4 || p.G == 8 || p.G == 16, "G=%d", p.G);
                    if (p.G != 1 && p.G != 4 && p.G != 8 && p.G != 16) continue;
                    CHECK((p.G == 1) == !k.groupwalk && !(p.fused && p.G == 1), "G=%d fused=%u", p.G, p.fused);
                    const uint64_t conns = PLAN_RX_THREADS / (uint32_t) p.G;
                    CHECK(p.tile == PLAN_RX_TILE && (uint64_t) p.tiles * p.tile >= n &&
                              (n == 0 ? p.tiles == 0 : (uint64_t) (p.tiles - 1) * p.tile < n),
                          "tiles=%u n=%u", p.tiles, n);
                    CHECK(p.emit_grid * conns >= n && (n == 0 ? p.emit_grid == 0 : (p.emit_grid - 1) * conns < n),
                          "emit_grid=%u n=%u G=%d", p.emit_grid, n, p.G);
                    CHECK(p.count_grid >= 1 && p.count_grid * conns >= (uint64_t) n + 1 &&
                              (p.count_grid - 1) * conns < (uint64_t) n + 1,
                          "count_grid=%u n=%u G=%d", p.count_grid, n, p.G);
                    const DtlsRxPlan d = dtls_rx_plan(n, m, k);
                    CHECK(d.fused == k.fused && (d.fused ? (d.S == 0 || d.S == 4 || d.S == 16) : d.S == -1) &&
                              (k.stash || d.S <= 0),
                          "S=%d fused=%u stash=%u", d.S, d.fused, k.stash);
                    CHECK((uint64_t) d.tiles * PLAN_DG_TILE >= n && (n == 0 ? d.tiles == 0 : (uint64_t) (d.tiles - 1) * PLAN_DG_TILE < n),
                          "dtls tiles=%u n=%u", d.tiles, n);
                    plans += 2;
                }
    printf("plan_sweep: %ld plans, %d failed\n", plans, fails);
    return fails ? 1 : 0;
}
