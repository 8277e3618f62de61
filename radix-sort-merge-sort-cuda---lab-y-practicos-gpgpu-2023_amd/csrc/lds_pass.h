// lds_pass.h -- the workgroup-wide 8-bit LSD passes over keys held in registers and LDS,
// shared by k_tile_sort (kernels.hip: one tile per workgroup) and block_sort_unit (lds_class.h:
// one segment or one row per workgroup, k_seg_block and k_rs_block).
#pragma once
#include "devutil.h"

namespace labsort {

template <int BLOCK, int KPT, bool KV = false>
struct TsSmem {
    static constexpr int R = 256, W = BLOCK / WAVE, TILE = BLOCK * KPT;
    static_assert(TILE <= 65536, "16-bit LDS slots");
    uint32_t keys[TILE];
    uint32_t vals[KV ? TILE : 1];  // key/value: the payload follows its key through every pass
    uint32_t whist[W * R];
    uint32_t wsum[W];
    uint32_t red_and[W];
    uint32_t red_or[W];
    uint32_t probe[WAVE];
    uint32_t ordered;
};

// Which of a wave's KPT 64-key groups hold keys.  pass() is taken once per digit pass; its
// result answers (use, j): does group j hold keys, asked where the pass ranks (use 0),
// stores (1) and reads back (2).  Wave-uniform.
struct AllGroups {  // every group: whole tiles, or tiles padded with sentinel keys
    struct Pass {
        __device__ __forceinline__ bool operator()(int, int) const { return true; }
    };
    __device__ __forceinline__ Pass pass() const { return {}; }
};
struct LeadingGroups {  // the first ng groups; the others are neither ranked, stored nor read back
    uint32_t ng;
    struct Pass {
        uint32_t n[3];
        __device__ __forceinline__ bool operator()(int use, int j) const { return (uint32_t)j < n[use]; }
    };
    // (the group count through an empty asm, one copy per use: the per-group compares are redone
    // where they are used; hoisted out of the pass loop they were held in SGPRs across it and spilled)
    __device__ __forceinline__ Pass pass() const {
        Pass p{{ng, ng, ng}};
        asm volatile("" : "+s"(p.n[0]), "+s"(p.n[1]), "+s"(p.n[2]));
        return p;
    }
};

// Sorts the workgroup's keys k (payloads v) by the digits in which they differ (`diff`: a
// pass whose digit is uniform is skipped: the reference's "stop when sorted", lab.cu:61,
// per tile), stably.  Wave `wid` holds LDS slots ws0 + j * 64 + lane in k[j], before and
// after; groups that `groups` leaves out keep their registers and must sort behind every
// ranked key (padding).  The caller's barrier separates the last use of sm.keys / sm.vals /
// sm.whist from this call; none follows the last read-back.
template <int BLOCK, int KPT, bool KV, class Groups>
__device__ __forceinline__ void lds_sort_passes(TsSmem<BLOCK, KPT, KV> &sm, uint32_t (&k)[KPT], uint32_t (&v)[KV ? KPT : 1],
                                                uint32_t diff, uint32_t flip, uint32_t ws0, bool atomic_rank,
                                                const Groups &groups, uint32_t lane, uint32_t wid) {
    using S = TsSmem<BLOCK, KPT, KV>;
    constexpr int R = S::R, W = S::W;
    uint32_t *wh = sm.whist + wid * R;
    for (int pass = 0; pass < 4; ++pass) {
        const uint32_t shift = pass * 8;
        if (((diff >> shift) & 0xFFu) == 0u) continue;  // uniform over the keys
        for (uint32_t i = lane; i < (uint32_t)R; i += WAVE) wh[i] = 0u;
        const auto holds = groups.pass();
        uint32_t rank[KPT / 2] = {};  // two 16-bit wave-local ranks, then LDS slots, per register
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            uint32_t r = 0u;
            if (holds(0, j)) r = rank8(wh, ((k[j] ^ flip) >> shift) & 0xFFu, lane, atomic_rank);
            set16(rank, j, r);
        }
        __syncthreads();
        fold_digit_offsets<BLOCK, W>(sm.whist, sm.wsum);
        __syncthreads();
        // every destination first (replacing its 16-bit rank: dst < TILE), the stores after:
        // interleaved, each counter read would wait for the store before it (the compiler
        // cannot tell the stores from the counters), 32 LDS round trips in a row per wave
#pragma unroll
        for (int j = 0; j < KPT; ++j) set16(rank, j, wh[((k[j] ^ flip) >> shift) & 0xFFu] + get16(rank, j));
        // (ranked slots number the keys and the padding of the last group: dst < TILE)
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (holds(1, j)) {
                const uint32_t dst = get16(rank, j);
                sm.keys[dst] = k[j];
                if constexpr (KV) sm.vals[dst] = v[j];
            }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (holds(2, j)) k[j] = sm.keys[ws0 + (uint32_t)j * WAVE + lane];
        if constexpr (KV) {
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if (holds(2, j)) v[j] = sm.vals[ws0 + (uint32_t)j * WAVE + lane];
        }
        // (the next pass's reorder writes sm.keys two barriers later)
    }
}

}  // namespace labsort
