/*
 * cbc_wave.hip -- the wave-per-record CBC + HMAC decryption kernel of
 * tlsrec_cbc_wave.h, instantiated for every (cipher, MAC) pair a slot can
 * hold: the decrypt side of the lane kernel's set (cbc.hip, cbc_alt.hip).
 * Only the coalesced single-record path launches it (engine.hip launch_cbc).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tlsrec.h"
#include "tlsrec_cbc.h"
#include "tlsrec_cbc_wave.h"
#include "tlsrec_internal.h"

using namespace tlsrec;

/* variants: as tlsrec__launch_cbc; identity order, a->perm is not read */
extern "C" hipError_t tlsrec__launch_cbc_wave(const CbcArgs *a, uint32_t variants, hipStream_t st)
{
    const uint32_t g = (uint32_t) ((a->n + CBC_WAVE_WAVES - 1) / CBC_WAVE_WAVES);
    if (g == 0) return hipSuccess;
    hipError_t e = hipSuccess;
#define TLSREC_CBC_LAUNCH(NR, CIPHER, MAC)                                                                          \
    if (e == hipSuccess && (variants & cbc_variant_bit(CIPHER, MAC))) {                                             \
        hipLaunchKernelGGL((tlsrec_cbc_wave_kernel<NR, MAC>), dim3(g), dim3(CBC_WAVE_THREADS), 0, st, *a);          \
        e = hipGetLastError();                                                                                      \
    }
    TLSREC_CBC_LAUNCH(10, TLSREC_CIPHER_AES_128_CBC, TLSREC_MAC_SHA1)
    TLSREC_CBC_LAUNCH(10, TLSREC_CIPHER_AES_128_CBC, TLSREC_MAC_SHA256)
    TLSREC_CBC_LAUNCH(10, TLSREC_CIPHER_AES_128_CBC, TLSREC_MAC_SHA384)
    TLSREC_CBC_LAUNCH(14, TLSREC_CIPHER_AES_256_CBC, TLSREC_MAC_SHA1)
    TLSREC_CBC_LAUNCH(14, TLSREC_CIPHER_AES_256_CBC, TLSREC_MAC_SHA256)
    TLSREC_CBC_LAUNCH(14, TLSREC_CIPHER_AES_256_CBC, TLSREC_MAC_SHA384)
    TLSREC_CBC_LAUNCH(12, TLSREC_CIPHER_ARIA_128_CBC, TLSREC_MAC_SHA256)
    TLSREC_CBC_LAUNCH(16, TLSREC_CIPHER_ARIA_256_CBC, TLSREC_MAC_SHA384)
    TLSREC_CBC_LAUNCH(18, TLSREC_CIPHER_CAMELLIA_128_CBC, TLSREC_MAC_SHA256)
    TLSREC_CBC_LAUNCH(24, TLSREC_CIPHER_CAMELLIA_256_CBC, TLSREC_MAC_SHA384)
#undef TLSREC_CBC_LAUNCH
    return e;
}
