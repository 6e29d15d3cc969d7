// pv_advance.h — the integer index arithmetic of the vocoder's phase increment, callable on the host as well as on the device,
// so that tests/host/pv_advance_check.cpp can hold it against the specification's formula for every bin and hop.
//
// The increment of bin k over an analysis hop of d samples is  adv + round(dw R / 2^24),  dw = qa - qp - e  (Q0.32, modulo 2^32), with the
// expected advance  e = ((k d) mod 1024) << 22.  Modulo 2^32 that is (k d) << 22 — the shift drops what the mask drops — hence
//   e(k + 64, d) = e(k, d) + (d << 28),   e(448 - k, d) = e(448, d) - e(k, d)   and   e(512, d) = d << 31.
// A plan has TWO hops: nae_stretch_plan sets d0 = floor(Ha) (ha_q24 >> 24) and frame f starts at round((f - 1) Ha) - N/2, so consecutive
// starts differ by d0 or d0 + 1, and r_q24[i] = round(2^24 H / (d0 + i)) is the ratio that goes with hop d0 + i.  So e is one of two per-bin
// constants, which the headline shape of the pipeline keeps in registers (pv_roles.h, PhaseLane::ea) instead of multiplying per frame and bin:
// a frame leaves  base = qa + e(k, d of the NEXT hop)  behind where it used to leave qa, and the next frame's deviation is qa - base.
// Any other d takes the general formula.
#pragma once
#include <stdint.h>
#include "../../include/nae_dsp_spec.h"

#if defined(__HIPCC__)
#define NAE_HD __host__ __device__ __forceinline__
#else
#define NAE_HD static inline
#endif

namespace nae {

// the specification's expected advance of bin k over a hop of d samples
NAE_HD uint32_t pv_expected_advance(unsigned k, unsigned d) { return ((k * d) & (NAE_FFT_N - 1)) << 22; }

// the same value without the mask; from bin k to bin k + 64; bin 512
NAE_HD uint32_t pv_advance_const(unsigned k, unsigned d) { return (k * d) << 22; }
NAE_HD uint32_t pv_advance_plus64(uint32_t e_k, unsigned d) { return e_k + (d << 28); }
NAE_HD uint32_t pv_advance_nyquist(unsigned d) { return d << 31; }
// bin 448 - k from bin k (the mirror pair's partner 64 bins down): (448 d) << 22 minus bin k's
NAE_HD uint32_t pv_advance_mirror448(uint32_t e_k, unsigned d) { return pv_advance_const(448u, d) - e_k; }

// the advance of bin k over hop d from the plan's two constants e_d0 = pv_advance_const(k, d0), e_d1 = pv_advance_const(k, d0 + 1)
NAE_HD uint32_t pv_advance_pick(unsigned k, unsigned d, unsigned d0, uint32_t e_d0, uint32_t e_d1)
{
    return d == d0 ? e_d0 : d == d0 + 1u ? e_d1 : pv_expected_advance(k, d);
}

// exact phase increment of one hop: adv + round(dw R / 2^24); the scaled deviation needs the exact 64-bit product
NAE_HD uint32_t pv_inc(uint32_t qa, uint32_t qp, uint32_t e, unsigned k, unsigned R)
{
    const int32_t dw = (int32_t)(qa - qp - e);
    const uint32_t adv = ((k * NAE_HOP) & (NAE_FFT_N - 1)) << 22;
    const long long scaled = ((long long)dw * (long long)(int32_t)R + (1ll << (NAE_R_FRAC_BITS - 1))) >> NAE_R_FRAC_BITS;
    return adv + (uint32_t)scaled;
}
// ... from base = qp + e, which the frame before left behind
NAE_HD uint32_t pv_inc_from_base(uint32_t qa, uint32_t base, unsigned k, unsigned R) { return pv_inc(qa, base, 0u, k, R); }

} // namespace nae
