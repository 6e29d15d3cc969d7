// chunk_stage.h — what every kernel that walks a stream in chunks shares (K11 kernels_eq.hip, K12 kernels_dyn.hip, K14 kernels_loud.hip, K15
// kernels_dynkey.hip, K16 kernels_echo.hip, K17 kernels_mod.hip): the tiling, the wave's LDS ordering, and the LDS stage a chunk passes through
// between its coalesced form in memory and the lanes' own samples ("K11 biquad cascade", "Kernel").
//
// A chunk is C = 64 T samples, T = 16 per lane.  In memory order 64 consecutive samples make one load or store of the wave; in lane order lane
// l owns samples [l T, l T + T).  The stage turns one into the other: sample n stands at word n + n / T, so a lane's T words are consecutive and
// two lanes' are T + 1 words apart, which is odd: the 32 lanes of a ds_read_b32 group fall on 32 different banks.
#pragma once
#include "launch.h"

namespace nae {

constexpr int kChunkT = 16, kChunkC = 64 * kChunkT, kChunkStride = kChunkT + 1;
constexpr int kChunkStage = kChunkC + 64;                  // words of a stage: chunk_word(kChunkC - 1) + 1 = kChunkC + 63, rounded up
static_assert(kChunkT == NAE_EQ_LANE && kChunkC == NAE_EQ_CHUNK && kChunkT == NAE_DYN_LANE && kChunkC == NAE_DYN_CHUNK,
              "DESIGN.md §3, K11 and K12: one tiling, chunks of 1024 samples, 16 per lane");

// the chunks that hold in_len samples: what a block entry walks
inline size_t nae_chunks(size_t in_len) { return (in_len + kChunkC - 1) / kChunkC; }

__device__ __forceinline__ void chunk_lds_sync()
{
    // this wave's LDS writes before its following LDS reads of other lanes' words: DS operations of one wave execute in issue order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// where sample n stands in a stage (n >= 0; of two chunks in a row too: dyn_walk's ring)
__device__ __forceinline__ int chunk_word(int n)
{
    static_assert(kChunkT == 16, "the shift is n / kChunkT");
    return n + (n >> 4);
}

// The coalesced load of the chunk at sample n0 of the signal at ip (samples fs apart, in_len of them, zero behind) into the stage, in one of two
// forms.  Guarded: a sample past in_len is not loaded.  Clamped: every load is issued, from an address inside the signal, and what lies past
// in_len is dropped behind it: loads in flight, not branches that each wait for their own.  UNROLL: the loads the compiler may keep together.
template <bool CLAMPED, int UNROLL>
__device__ __forceinline__ void chunk_load(float* stage, const float* ip, long long fs, long long n0, long long in_len, int lane)
{
#pragma unroll UNROLL
    for (int j = 0; j < kChunkT; j++) {
        const int n = j * 64 + lane;
        const long long g = n0 + n;
        if constexpr (CLAMPED) {
            const float v = ip[(g < in_len ? g : in_len - 1) * fs];   // always a sample of the signal: no branch
            stage[chunk_word(n)] = g < in_len ? v : 0.0f;
        } else {
            stage[chunk_word(n)] = g < in_len ? ip[g * fs] : 0.0f;
        }
    }
}

// the coalesced store of the staged chunk at sample n0 to op: samples at or past in_len are not stored
template <int UNROLL>
__device__ __forceinline__ void chunk_store(const float* stage, float* op, long long fs, long long n0, long long in_len, int lane)
{
#pragma unroll UNROLL
    for (int j = 0; j < kChunkT; j++) {
        const int n = j * 64 + lane;
        const long long g = n0 + n;
        if (g < in_len) op[g * fs] = stage[chunk_word(n)];
    }
}

// the lane's own T samples out of the stage (X: float, or double for a recurrence kept in double) and back into it, rounded to f32
template <class X>
__device__ __forceinline__ void chunk_lane_read(const float* stage, int lane, X* x)
{
#pragma unroll
    for (int k = 0; k < kChunkT; k++) x[k] = (X)stage[lane * kChunkStride + k];
}

template <class X>
__device__ __forceinline__ void chunk_lane_write(float* stage, int lane, const X* x)
{
#pragma unroll
    for (int k = 0; k < kChunkT; k++) stage[lane * kChunkStride + k] = (float)x[k];
}

} // namespace nae
