// fin_block.h -- k_fin_block, the block class of the hybrid radix sort's finish (segsort.hip,
// DESIGN.md §3.9): one 256-thread workgroup per bucket of the top 16 bits, 1 .. HY_BLOCK_KEYS keys.
//
// It is k_seg_block + lds_sort_passes (lds_pass.h) cut down to what this caller needs.  The
// bucket's keys share their top two digits (the scatter passes ordered them) and nothing is known
// about the low two, so the two LDS passes on digits 0 and 1 always run and no reduction looks for
// the digits that vary: a pass over a digit that is uniform inside one bucket moves every key to
// where it was.  Each wave folds the W waves' counters into its own 256 offsets (four digits per
// lane, a scan across the wave) instead of 256 threads folding for everybody between two workgroup
// barriers, so a pass has two workgroup barriers, a bucket four.  The next bucket's keys are loaded
// while the last pass's result still sits in LDS, so they are under way before this bucket's
// stores and arrive while those drain.
#pragma once
#include "segsort.h"

#include "devutil.h"

namespace labsort {

namespace {

// LABSORT_FIN_PREFETCH=0: load a bucket's keys when its turn comes (A/B builds).
#ifndef LABSORT_FIN_PREFETCH
#define LABSORT_FIN_PREFETCH 1
#endif
// List entries granted per ticket.  One per ticket is 65536 returning adds on one word in the
// kernel's 0.56 ms, more than the word takes (one per 12.5 ns): the finish of 2^28 uniform keys ran
// 0.816 ms against 0.562 with two and 0.560 with four (A/B builds, DESIGN.md §3.9,
// profiles/fin_tickets_ab.txt).  Four also leaves room for lists of the class's shortest buckets.
#ifndef LABSORT_FIN_GRANT
#define LABSORT_FIN_GRANT 4
#endif
constexpr int FIN_GRANT = LABSORT_FIN_GRANT;
static_assert(FIN_GRANT >= 1, "a ticket grants at least one entry");

// Inclusive scan over the wave in registers: four row shifts scan each row of 16 lanes, the two
// row broadcasts of gfx9 carry lane 15 into the next row and lane 31 into the upper half (six
// ds_bpermute round trips as shuffles, and their six lane addresses held in registers).
__device__ __forceinline__ uint32_t wave_incl_scan_dpp(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    return x;
}

template <int BLOCK, int KPT>
struct FinSmem {
    static constexpr int R = 256, W = BLOCK / WAVE, TILE = BLOCK * KPT;
    static_assert(TILE <= 65536, "16-bit LDS slots");
    static_assert(W == 4, "the fold holds one counter row per wave in registers");
    uint32_t keys[TILE];
    alignas(16) uint32_t cnt[W * R];   // cnt[w * 256 + d]: wave w's count of digit d
    alignas(16) uint32_t offs[W * R];  // offs[w * 256 + d]: first slot of wave w's keys of digit d; wave w's own
    uint32_t probe[WAVE];
    uint32_t ordered;
    uint32_t tick[2];  // the ticket thread 0 drew, by the iteration's parity (k_fin_block)
};

// A bucket [b, b + len) striped over the W waves as block_stripe (lds_class.h) stripes a unit.  Wave-uniform
// but tail_ok.  (The arithmetic stands here a second time: through block_stripe the kernel gained four
// scalar instructions and bench.py's headline read 0.2-0.5 % higher in four sessions of four)
struct FinStripe {
    size_t sb;     // b + ws0: the stripe's first key in global memory
    uint32_t ws0;  // its first LDS slot
    uint32_t nf;   // whole groups
    uint32_t ng;   // groups that hold keys: nf, or nf + 1 with a last group of 1-63 keys
    bool tail_ok;  // this lane holds a key of that last group
};
template <int W, int KPT>
__device__ __forceinline__ FinStripe fin_stripe(uint32_t b, uint32_t len, uint32_t lane, uint32_t wid) {
    if (len > (uint32_t)(W * WAVE * KPT)) len = 0u;  // (never listed in this class: touch nothing)
    const uint32_t jn = (len + (uint32_t)(W * WAVE) - 1u) / (uint32_t)(W * WAVE);  // <= KPT
    const uint32_t ws0 = wid * jn * WAVE;
    const uint32_t rem = ws0 < len ? len - ws0 : 0u;
    const uint32_t nf = min(jn, rem / WAVE);
    const uint32_t tail = nf < jn ? rem - nf * WAVE : 0u;  // < 64
    return {(size_t)b + ws0, ws0, nf, nf + (tail ? 1u : 0u), lane < tail};
}

// The stripe's keys, all loads in flight together.  Padding is all ones: digit 0xFF in both
// passes, and it starts behind every key in slot order, so the stable passes leave it behind
// every key, one that ends in 0xFFFF included.
template <int KPT>
__device__ __forceinline__ void fin_load(const uint32_t *in, const FinStripe &g, uint32_t lane, uint32_t (&k)[KPT]) {
    // a wave-uniform base and a 32-bit byte offset per access (lane and group: below 2^15, so the
    // group's part goes into the instruction's offset field): one per-lane address for all loads
    const char *pb = reinterpret_cast<const char *>(in + g.sb);
    const uint32_t lb = lane * 4u;
    if (g.nf == (uint32_t)KPT) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) k[j] = ld_stream<NT_TILE>(reinterpret_cast<const uint32_t *>(pb + (lb + (uint32_t)(j * WAVE * 4))));
    } else {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            k[j] = 0xFFFFFFFFu;
            if ((uint32_t)j < g.nf || ((uint32_t)j == g.nf && g.tail_ok))
                k[j] = ld_stream<NT_TILE>(reinterpret_cast<const uint32_t *>(pb + (lb + (uint32_t)(j * WAVE * 4))));
        }
    }
}

// One stable 8-bit pass over the workgroup's keys, up to the barrier behind the reorder stores:
// on return sm.keys holds them in the new order.
template <int BLOCK, int KPT>
__device__ __forceinline__ void fin_pass(FinSmem<BLOCK, KPT> &sm, const uint32_t (&k)[KPT], uint32_t shift, uint32_t ng,
                                         bool atomic_rank, uint32_t lane, uint32_t wid) {
    constexpr int W = FinSmem<BLOCK, KPT>::W, R = FinSmem<BLOCK, KPT>::R;
    uint32_t *wh = sm.cnt + wid * R;
    uint32_t *wo = sm.offs + wid * R;
    // (one copy of the group count per use: hoisted compares were held in SGPRs across the pass)
    uint32_t n0 = ng, n1 = ng;
    asm volatile("" : "+s"(n0), "+s"(n1));
    // (the zero through an empty asm: as a loop invariant four zero registers were kept across the
    // bucket loop, spilled, and reloaded behind a wait for every global access)
    uint32_t z = 0u;
    asm volatile("" : "+v"(z));
    *reinterpret_cast<uint4 *>(wh + 4u * lane) = make_uint4(z, z, z, z);
    uint32_t rank[KPT / 2] = {};  // two 16-bit wave-local ranks, then LDS slots, per register
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        uint32_t r = 0u;
        if ((uint32_t)j < n0) r = rank8(wh, (k[j] >> shift) & 0xFFu, lane, atomic_rank);
        set16(rank, j, r);
    }
    __syncthreads();  // (A)
    {
        // this lane's four digits 4 lane .. 4 lane + 3: their counts in every wave, the keys of
        // the digits before them by a scan across the wave, and from both the first slot of
        // this wave's keys of each
        uint4 c[W];
#pragma unroll
        for (int w = 0; w < W; ++w) c[w] = *reinterpret_cast<const uint4 *>(sm.cnt + w * R + 4u * lane);
        uint32_t tot[4] = {0u, 0u, 0u, 0u}, bef[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t cw[4] = {c[w].x, c[w].y, c[w].z, c[w].w};
            const bool before = (uint32_t)w < wid;  // wave-uniform
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                tot[q] += cw[q];
                bef[q] += before ? cw[q] : 0u;
            }
        }
        const uint32_t s = tot[0] + tot[1] + tot[2] + tot[3];
        uint32_t run = wave_incl_scan_dpp(s) - s;
        uint4 o4;
        o4.x = run + bef[0];
        run += tot[0];
        o4.y = run + bef[1];
        run += tot[1];
        o4.z = run + bef[2];
        run += tot[2];
        o4.w = run + bef[3];
        *reinterpret_cast<uint4 *>(wo + 4u * lane) = o4;
    }
    __builtin_amdgcn_wave_barrier();
    // every destination first (replacing its 16-bit rank: dst < TILE, the ranked slots number the
    // keys and the padding of the last group), the stores after: interleaved, each offset read
    // would wait for the store before it.  Groups without keys read no offset.
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if ((uint32_t)j < n1) set16(rank, j, wo[(k[j] >> shift) & 0xFFu] + get16(rank, j));
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if ((uint32_t)j < n1) sm.keys[get16(rank, j)] = k[j];
    __syncthreads();  // (B)
}

// Workgroup barriers: (A) after the rank and (B) after the reorder stores of each pass, nothing
// else, and none between buckets:
//  * sm.cnt row w is zeroed and added to by wave w only, and read by every wave's fold between
//    (A) and (B) of the same pass.  Wave w zeroes it again behind (B), which every wave reaches
//    after its fold.
//  * sm.offs row w is written and read by wave w alone, in program order (LDS operations of one
//    wave complete in issue order).
//  * sm.keys is stored to between (A) and (B) and read back behind (B).  The next stores, of the
//    next pass or the next bucket, come behind the next (A), which a wave reaches only after its
//    read-back has returned.
template <int BLOCK, int KPT, int WPE>
__global__ __launch_bounds__(BLOCK, WPE) void k_fin_block(uint32_t *out, const uint32_t *__restrict__ off,
                                                           const uint32_t *__restrict__ hdr,
                                                           const uint32_t *__restrict__ list, uint32_t *ticket, HySel hy) {
    using S = FinSmem<BLOCK, KPT>;
    constexpr int W = S::W;
    constexpr int CLS = 3;
    constexpr bool PREFETCH = LABSORT_FIN_PREFETCH != 0;
    __shared__ S sm;
    if (hy.plan->hybrid == 0u) return;  // the classic path was chosen
    const uint32_t *in = hy.buf[hy.plan->fin_src];
    if (ld_agent(hdr) != 0u) return;  // rejected offsets: touch nothing
    const uint32_t cnt = hdr[SEG_HDR_CNT + CLS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (blockIdx.x >= cnt) return;  // (an empty class costs its launch only; uniform over the workgroup)
    // The list is handed out by ticket (hdr[SEG_HDR_TICKET], zero at launch): entry blockIdx.x is
    // this workgroup's first, every later one comes from a grant of FIN_GRANT consecutive entries
    // from gridDim.x + FIN_GRANT * ticket on, so a workgroup that runs slow takes fewer buckets and
    // nobody waits for anybody.  Thread 0 draws; the grant reaches the other waves through sm.tick.
    // `nxt` is the entry after the one being sorted (>= cnt: none), `left` the entries of its grant
    // behind it.  The first draw is waited for at the probe's barrier, once per workgroup.
    const bool any_more = cnt > gridDim.x;  // else the first entries are all there is: no draw
    if (any_more && tid == 0u) sm.tick[1] = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    probe_lane_order(sm.probe, &sm.ordered, lane, wid);
    __syncthreads();
    const bool atomic_rank = lane_order_probed(&sm.ordered);
    uint32_t nxt = any_more ? gridDim.x + (uint32_t)FIN_GRANT * __builtin_amdgcn_readfirstlane(sm.tick[1]) : cnt;
    uint32_t left = (uint32_t)FIN_GRANT - 1u;
    // the list entry and the two offsets are three dependent loads: those of the bucket after
    // the next are issued before this one is sorted
    uint32_t nb, ne;
    {
        const uint32_t seg = __builtin_amdgcn_readfirstlane(list[blockIdx.x]);
        nb = __builtin_amdgcn_readfirstlane(off[seg]);
        ne = __builtin_amdgcn_readfirstlane(off[seg + 1]);
    }
    uint32_t k[KPT];
    FinStripe g = fin_stripe<W, KPT>(nb, ne - nb, lane, wid);
    if constexpr (PREFETCH) fin_load(in, g, lane, k);
    for (uint32_t it = blockIdx.x, par = 0u; it < cnt; par ^= 1u) {
        if constexpr (!PREFETCH) {
            g = fin_stripe<W, KPT>(nb, ne - nb, lane, wid);
            fin_load(in, g, lane, k);
        }
        const bool more = nxt < cnt;
        // the entry after the next: the next one of the same grant, or a draw, issued here and not
        // waited for before the second pass (workgroup-uniform)
        const bool draw = more && (FIN_GRANT == 1 || left == 0u);
        uint32_t drawn = 0u;
        if (draw && tid == 0u) drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (more) {
            const uint32_t seg = __builtin_amdgcn_readfirstlane(list[nxt]);
            nb = __builtin_amdgcn_readfirstlane(off[seg]);
            ne = __builtin_amdgcn_readfirstlane(off[seg + 1]);
        }
        fin_pass(sm, k, 0u, g.ng, atomic_rank, lane, wid);
        {
            uint32_t n2 = g.ng;
            asm volatile("" : "+s"(n2));
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if ((uint32_t)j < n2) k[j] = sm.keys[g.ws0 + (uint32_t)j * WAVE + lane];
        }
        // the drawn ticket: stored before the second pass's barriers, read behind them; two words
        // by the iteration's parity, so the next store never meets a wave still reading this one
        if (draw && tid == 0u) sm.tick[par] = drawn;
        fin_pass(sm, k, 8u, g.ng, atomic_rank, lane, wid);
        it = nxt;
        if (draw) {
            nxt = gridDim.x + (uint32_t)FIN_GRANT * __builtin_amdgcn_readfirstlane(sm.tick[par]);
            left = (uint32_t)FIN_GRANT - 1u;
        } else {
            nxt += 1u;  // (no more entries: past cnt, as it is)
            left -= 1u;
        }
        // the sorted bucket is in sm.keys and k is free: the next bucket's loads go out first
        FinStripe gn = g;
        uint32_t kn[PREFETCH ? KPT : 1];
        if constexpr (PREFETCH) {
            gn = fin_stripe<W, KPT>(nb, more ? ne - nb : 0u, lane, wid);
            fin_load(in, gn, lane, kn);
        }
        uint32_t nfs = g.nf;
        asm volatile("" : "+s"(nfs));
        const uint32_t *sk = sm.keys + g.ws0 + lane;
        char *ob = reinterpret_cast<char *>(out + g.sb);
        const uint32_t lb = lane * 4u;
        if (nfs == (uint32_t)KPT) {
#pragma unroll
            for (int j = 0; j < KPT; ++j) *reinterpret_cast<uint32_t *>(ob + (lb + (uint32_t)(j * WAVE * 4))) = sk[j * WAVE];
        } else {
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if ((uint32_t)j < nfs || ((uint32_t)j == nfs && g.tail_ok))
                    *reinterpret_cast<uint32_t *>(ob + (lb + (uint32_t)(j * WAVE * 4))) = sk[j * WAVE];
        }
        if constexpr (PREFETCH) {
            g = gn;
#pragma unroll
            for (int j = 0; j < KPT; ++j) k[j] = kn[j];
        }
    }
}

}  // namespace

}  // namespace labsort
