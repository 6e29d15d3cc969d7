// eq_cascade.h — what the kernels that run a biquad cascade share (K11 kernels_eq.hip, K14 kernels_loud.hip, K15 kernels_dynkey.hip, K16
// kernels_echo.hip): the layout of a cascade's constant block, the copy of its p and q into LDS, the sections' carry in and out, and one section
// of the tiled form on a lane's 16 samples ("K11 biquad cascade", steps 1, 3 and 4).  The tiling and the LDS stage stand in
// chunk_stage.h.  The translation units are built with -ffp-contract=off: every step is one IEEE operation, in the order of tests/eq_ref/ref_eq.c.
#pragma once
#include "chunk_stage.h"

namespace nae {

constexpr int kEqCoefs = 5, kEqTab = 2 * kChunkT + 6 * 4;  // per section: b0 b1 b2 a1 a2 | p[T] q[T] Phi_0 ... Phi_5 (m00 m01 m10 m11 each)
constexpr int kEqTabOfs = NAE_EQ_MAX_SECTIONS * kEqCoefs;  // the tables stand behind the coefficients of all sections
constexpr size_t kEqBlockDoubles = (size_t)NAE_EQ_MAX_SECTIONS * (kEqCoefs + kEqTab);
static_assert(kEqTab == 56, "DESIGN.md §3, K11: 56 doubles of tables per section");

// p and q of the first n_sections sections out of the constant block into pq[n_sections][2 T] in LDS, by thread tid of `threads`; the caller
// orders the copy in front of the sections' reads
__device__ __forceinline__ void eq_stage_pq(double* pq, const double* __restrict__ tab, int n_sections, int tid, int threads)
{
    for (int i = tid; i < n_sections * 2 * kChunkT; i += threads) pq[i] = tab[kEqTabOfs + (i / (2 * kChunkT)) * kEqTab + (i % (2 * kChunkT))];
}

// The carry of the S sections of stream-channel sc in state[n_sc][max_sections][2]: lane s keeps section s's (z1, z2).  state null: zero in,
// nothing out.
__device__ __forceinline__ void eq_carry_load(const double* state, long long sc, int max_sections, int lane, int S, double& st1, double& st2)
{
    st1 = st2 = 0.0;
    if (state && lane < S) {
        st1 = state[(sc * max_sections + lane) * 2];
        st2 = state[(sc * max_sections + lane) * 2 + 1];
    }
}

__device__ __forceinline__ void eq_carry_store(double* state, long long sc, int max_sections, int lane, int S, double st1, double st2)
{
    if (state && lane < S) {
        state[(sc * max_sections + lane) * 2] = st1;
        state[(sc * max_sections + lane) * 2 + 1] = st2;
    }
}

// Section s over the lane's samples x (in: the section's input, out: its output, both as doubles).  tab: the constant block; pq: p and q of
// every section in LDS (read at wave-uniform addresses: a broadcast).  Lane s holds the section's carry (st1, st2) between chunks: it is
// read by a broadcast and replaced by the scan's last value.
__device__ __forceinline__ void eq_section(double (&x)[kChunkT], int s, int lane, const double* __restrict__ tab, const double* pq, double& st1, double& st2)
{
    const double* cf = tab + s * kEqCoefs;
    const double* t = pq + s * 2 * kChunkT;
    const double b0 = cf[0], b1 = cf[1], b2 = cf[2], a1 = cf[3], a2 = cf[4];
    // 1: the zero-state pass
    double z1 = 0.0, z2 = 0.0;
#pragma unroll
    for (int k = 0; k < kChunkT; k++) {
        const double xv = x[k];
        const double y = b0 * xv + z1;
        z1 = (b1 * xv - a1 * y) + z2;
        z2 = b2 * xv - a2 * y;
        x[k] = y;
    }
    // 3: the carry.  E_0 takes the chunk's carry-in, then six steps, each reading the previous step's values
    const double in1 = __shfl(st1, s), in2 = __shfl(st2, s);
    const double* ph = tab + kEqTabOfs + s * kEqTab + 2 * kChunkT;
    if (lane == 0) {
        const double e1 = z1 + ((ph[0] * in1) + (ph[1] * in2));
        const double e2 = z2 + ((ph[2] * in1) + (ph[3] * in2));
        z1 = e1;
        z2 = e2;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const double u1 = __shfl_up(z1, 1u << j), u2 = __shfl_up(z2, 1u << j);
        const double e1 = z1 + ((ph[4 * j] * u1) + (ph[4 * j + 1] * u2));
        const double e2 = z2 + ((ph[4 * j + 2] * u1) + (ph[4 * j + 3] * u2));
        if (lane >= (1 << j)) {
            z1 = e1;
            z2 = e2;
        }
    }
    double s1 = __shfl_up(z1, 1u), s2 = __shfl_up(z2, 1u);
    if (lane == 0) {
        s1 = in1;
        s2 = in2;
    }
    const double o1 = __shfl(z1, 63), o2 = __shfl(z2, 63);
    if (lane == s) {
        st1 = o1;
        st2 = o2;
    }
    // 4: the correction; y is the next section's input
#pragma unroll
    for (int k = 0; k < kChunkT; k++) x[k] = x[k] + ((t[k] * s1) + (t[kChunkT + k] * s2));
}

} // namespace nae

// kernels_eq.hip: the constant block of `n_sections` checked sections coef[n][5] into blk[kEqBlockDoubles] on the host ("K11
// biquad cascade", step 2: p, q and the six maps in double-double, rounded to double once)
void eq_make_tables(const double* coef, int n_sections, double* blk);
