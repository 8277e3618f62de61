// hist_lean.hip -- k_hist_lean, the hybrid radix sort's own upfront count.
//
// A hybrid sort (scatter passes on digits 2 and 3, buckets of the top 16 bits finished in LDS)
// needs two counts per key, not the five of k_hist_seg<true>: digit 2 per position segment
// (hy.hps2, the first pass's chains) and the top 14 bits (hy.top14: the bucket bound, the
// finish's offsets and, summed in fours, the digit-3 pass's segment plan).  Whether digits 0 and 1
// vary comes from the AND and the OR of the keys.  This kernel counts just that, and its last
// workgroup to finish evaluates k_plan8's rule on the exact counts and stores the verdict.
//
// Which count runs first is a prediction from a fixed sample of the keys; the path is never
// decided by it.  Sequence (api.hip's sort_radix8): k_hist_lean, k_hist_seg<true>, k_plan8.
//   sample says "hybrid unlikely": k_hist_lean returns at once, no verdict; the full count runs
//                                   and k_plan8 decides as it always did;
//   verdict hybrid:                 the full count returns at once;
//   verdict classic (mispredicted): the full count runs after all, and k_plan8 takes the verdict.
// A kernel of its own module: kernels.hip's kernels keep their registers and LDS.
#include "common.h"
#include "devutil.h"

namespace labsort {

namespace {

// The sample: HY_SAMPLE_RUNS runs of 64 consecutive keys, one run per 1/256th of the input at an
// offset that depends on the run only, so every workgroup (and every call at this n) reads the
// same keys; after the first workgroup of an XCD they come from its L2.
constexpr uint32_t HY_SAMPLE_RUNS = 256, HY_SAMPLE_RUN = 64, HY_SAMPLE = HY_SAMPLE_RUNS * HY_SAMPLE_RUN;
constexpr uint32_t HY_COARSE_BITS = 4, HY_COARSE = 1u << HY_COARSE_BITS;  // bins of the sample's top bits
static_assert(HY_SAMPLE == 16 * HIST_BLOCK, "16 sample keys per thread, one run per wave and round");

// "Hybrid likely"?  Unlikely when digit 0 or digit 1 is the same in every sampled key, or when a
// sixteenth of the key space holds so many sampled keys that, scaled to n, its 1024 top-14-bit
// groups average above 1.25 x limit.  Uniform keys put 1024 +- 31 of the 16384 sampled keys into a
// bin: at 19 x 2^24 keys (mean group 19456, limit 20480) the threshold is 1347 keys, 10 standard
// deviations up; 2^28 keys below 2^31 put 2048 +- 42 into each of eight bins against a
// threshold of 1600, 10 standard deviations down.  sc: 32 * HY_COARSE + 2 words of LDS.
// Every thread returns the same answer.  Needs n >= HY_SAMPLE.
__device__ bool predict_hybrid(const uint32_t *__restrict__ keys, size_t n, uint32_t flip, uint32_t limit, uint32_t *sc) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wid = t >> 6;
    uint32_t *sand = sc + 32 * HY_COARSE, *sor = sand + 1;
    if (t < 32 * HY_COARSE) sc[t] = 0u;
    if (t == 0) {
        *sand = ~0u;
        *sor = 0u;
    }
    __syncthreads();
    const size_t span = n / HY_SAMPLE_RUNS;  // >= 64
    const uint32_t room = (uint32_t)(span - (HY_SAMPLE_RUN - 1));
    uint32_t x[16];
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t r = j * 16u + wid;
        const size_t pos = (size_t)r * span + ((r * 2654435761u) >> 8) % room + lane;
        x[j] = keys[pos];
    }
    uint32_t a = ~0u, o = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t k = x[j] ^ flip;
        a &= k;
        o |= k;
        atomicAdd(&sc[(k >> (32 - HY_COARSE_BITS)) * 32u + (lane & 31u)], 1u);  // replicated: no lane waits for another
    }
    wave_and_or(a, o);
    if (lane == 0) {
        atomicAnd(sand, a);
        atomicOr(sor, o);
    }
    __syncthreads();
    uint32_t c = 0;
    if (t < 64u) {  // wave 0: bin t >> 2, a quarter of its slots each
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) c += sc[(t >> 2) * 32u + (t & 3u) * 8u + q];
        c += __shfl_xor(c, 1);
        c += __shfl_xor(c, 2);
#pragma unroll
        for (int off = 4; off < 64; off <<= 1) c = max(c, (uint32_t)__shfl_xor(c, off));
    }
    const uint32_t diff = *sand ^ *sor;
    __syncthreads();
    if (t == 0) sc[0] = c;
    __syncthreads();
    const uint32_t maxc = sc[0];
    __syncthreads();  // (sc is the caller's again)
    if ((diff & 255u) == 0u || ((diff >> 8) & 255u) == 0u) return false;
    const uint64_t groups = HY_TOP >> HY_COARSE_BITS;  // top-14-bit groups in one bin
    return (uint64_t)maxc * n * 4u <= (uint64_t)5u * limit * HY_SAMPLE * groups;
}

}  // namespace

// Grid and key ranges as k_hist_seg: NSEG * bps workgroups, each reading one part of one
// position segment with software-pipelined 16-byte loads.  Two LDS atomics per key: digit 2 in SL
// replicated counters, the top 14 bits plain; a value repeated over a wave, a lane's 16 keys
// or a uint4 is added once (k_hist_seg's add_field: sorted or clustered keys would otherwise
// serialise on one counter).  The AND and OR of key ^ flip stay in registers.
// ctl words (the workspace's zeroed header, common.h): the ticket, ~AND, OR, the verdict, "ran".
template <int SL>
__global__ __launch_bounds__(HIST_BLOCK) void k_hist_lean(const uint32_t *__restrict__ keys, size_t n, uint32_t flip,
                                                          uint32_t *__restrict__ joint, uint32_t bps, HyCounts hy) {
    static_assert(256 * SL >= 32 * (int)HY_COARSE + 2, "the sample's counters fit the digit-2 counters");
    __shared__ uint32_t h2[256 * SL];
    __shared__ uint32_t ht[HY_TOP];
    __shared__ uint32_t red[4];  // AND, OR, largest top14 count, last-workgroup flag
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (hy.mode == HY_COUNT_FULL) return;
    if (hy.mode != HY_COUNT_LEAN && !predict_hybrid(keys, n, flip, hy.limit, h2)) return;
    if (blockIdx.x == 0 && t == 0) hy.ctl[HY_CTL_LEAN] = 1u;
    for (int i = t; i < 256 * SL; i += HIST_BLOCK) h2[i] = 0u;
    for (int i = t; i < HY_TOP; i += HIST_BLOCK) ht[i] = 0u;
    if (t == 0) {
        red[0] = ~0u;
        red[1] = 0u;
        red[2] = 0u;
    }
    __syncthreads();
    constexpr int NU = 4;  // uint4 loads in flight per thread, counted 16 keys at a time (8 in flight: 254 us against 244)
    const uint32_t slot = t & (SL - 1);
    uint32_t ka = ~0u, ko = 0u;
    auto dig2 = [&](uint32_t k) { return (k >> 16) & 255u; };
    auto top = [&](uint32_t k) { return k >> (32 - HY_TOP_BITS); };
    auto count = [&](uint32_t k) {
        k ^= flip;
        ka &= k;
        ko |= k;
        atomicAdd(&h2[dig2(k) * SL + slot], 1u);
        atomicAdd(&ht[top(k)], 1u);
    };
    auto count16 = [&](const uint4 (&c)[4]) {
        uint32_t k[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            k[4 * u] = c[u].x ^ flip;
            k[4 * u + 1] = c[u].y ^ flip;
            k[4 * u + 2] = c[u].z ^ flip;
            k[4 * u + 3] = c[u].w ^ flip;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            ka &= k[j];
            ko |= k[j];
        }
        // as k_hist_seg: the repeat tests run only in waves where some lane's top field repeats
        // within its first uint4, so uniform keys keep the plain adds
        if (__ballot(top(k[0]) == top(k[3])) == 0ull) {
#pragma unroll
            for (int j = 0; j < 16; ++j) atomicAdd(&h2[dig2(k[j]) * SL + slot], 1u);
#pragma unroll
            for (int j = 0; j < 16; ++j) atomicAdd(&ht[top(k[j])], 1u);
            return;
        }
        auto add_field = [&](auto &&fv, auto &&ctr) {
            const uint32_t f0 = fv(k[0]);
            bool same = fv(k[15]) == f0;
            if (same) {
#pragma unroll
                for (int j = 1; j < 15; ++j) same &= fv(k[j]) == f0;
            }
            const uint32_t w0 = __builtin_amdgcn_readfirstlane(f0);
            const uint64_t act = __ballot(true);
            if (__ballot(same && f0 == w0) == act) {  // the whole wave on one value
                if (mbcnt64(act) == 0u) atomicAdd(ctr(w0), 16u * (uint32_t)__popcll(act));
                return;
            }
            if (same) {
                atomicAdd(ctr(f0), 16u);
                return;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t fa = fv(k[4 * u]);
                const bool s4 = fv(k[4 * u + 3]) == fa && fv(k[4 * u + 1]) == fa && fv(k[4 * u + 2]) == fa;
                if (s4) {
                    atomicAdd(ctr(fa), 4u);
                } else {
#pragma unroll
                    for (int j = 4 * u; j < 4 * u + 4; ++j) atomicAdd(ctr(fv(k[j])), 1u);
                }
            }
        };
        add_field(dig2, [&](uint32_t f) { return &h2[f * SL + slot]; });
        add_field(top, [&](uint32_t f) { return &ht[f]; });
    };
    const uint32_t seg = blockIdx.x / bps, part = blockIdx.x % bps;
    const size_t sb = seg_start(seg, n), se = seg_start(seg + 1, n);
    const size_t per = (se - sb + bps - 1) / bps;
    const size_t beg = sb + (size_t)part * per < se ? sb + (size_t)part * per : se;
    const size_t end = beg + per < se ? beg + per : se;
    if ((((uintptr_t)keys) & 15u) == 0) {
        // scalar head up to 16-B alignment, uint4 body, scalar tail
        const size_t abeg = (beg + 3) & ~(size_t)3;
        const size_t vbeg = abeg < end ? abeg : end;
        for (size_t i = beg + t; i < vbeg; i += HIST_BLOCK) count(keys[i]);
        const size_t nv = (end - vbeg) / 4;
        const uint4 *v = reinterpret_cast<const uint4 *>(keys + vbeg);
        size_t i = t;
        uint4 c[NU], x[NU];  // the next NU x uint4 load while the current ones are counted
        if (i + (NU - 1) * HIST_BLOCK < nv) {
#pragma unroll
            for (int u = 0; u < NU; ++u) c[u] = ld_stream4<NT_HIST>(v + i + u * HIST_BLOCK);
        }
        for (; i + (NU - 1) * HIST_BLOCK < nv; i += NU * HIST_BLOCK) {
            if (i + (2 * NU - 1) * HIST_BLOCK < nv) {
#pragma unroll
                for (int u = 0; u < NU; ++u) x[u] = ld_stream4<NT_HIST>(v + i + (NU + u) * HIST_BLOCK);
            }
            count16(c);
#pragma unroll
            for (int u = 0; u < NU; ++u) c[u] = x[u];
        }
        for (; i < nv; i += HIST_BLOCK) {
            const uint4 y = ld_stream4<NT_HIST>(v + i);
            count(y.x); count(y.y); count(y.z); count(y.w);
        }
        for (size_t r = vbeg + nv * 4 + t; r < end; r += HIST_BLOCK) count(keys[r]);
    } else {
        for (size_t i = beg + t; i < end; i += HIST_BLOCK) count(keys[i]);
    }
    wave_and_or(ka, ko);
    if (lane == 0) {
        atomicAnd(&red[0], ka);
        atomicOr(&red[1], ko);
    }
    __syncthreads();
    if (t < 256u) {
        uint32_t c = 0;
#pragma unroll 8
        for (int q = 0; q < SL; ++q) c += h2[t * SL + ((q + t) & (SL - 1))];
        if (c) atomicAdd(&hy.hps2[seg * 256 + t], c);
    }
    // each workgroup starts its flush at a different place (as k_hist_seg's)
    const uint32_t rot = (blockIdx.x * 1088u) & (uint32_t)(HY_TOP - 1);
    for (uint32_t i0 = t; i0 < (uint32_t)HY_TOP; i0 += HIST_BLOCK) {
        const uint32_t i = (i0 + rot) & (uint32_t)(HY_TOP - 1);
        const uint32_t c = ht[i];
        if (c) atomicAdd(&hy.top14[i], c);
    }
    if (t == 0) {  // (a workgroup without keys adds nothing: ~AND = OR = 0)
        atomicOr(&hy.ctl[HY_CTL_NAND], ~red[0]);
        atomicOr(&hy.ctl[HY_CTL_OR], red[1]);
    }
    // The last workgroup to get here evaluates the rule: everyone's counts are out before
    // their ticket is drawn, and nobody waits for anybody.  Every wave waits until its own count
    // atomics (returnless device-scope RMWs, counted by vmcnt) have been performed -- the
    // barrier's workgroup-scope release does not emit that wait -- then the barrier, then
    // thread 0 alone fences at device scope and draws the ticket.  A fence in every thread is
    // an L2 write-back and invalidate per wave, 4096 of them while other workgroups still
    // stream, and cost 0.07 ms of the kernel's 0.24 (harness/exp/lean_count_probe.hip FENCE 3
    // is this shape; profiles/count_pipeline_probe.txt, count_pipeline_isa.txt).
    // (the immediate is the gfx9 encoding, gfx950 included: vmcnt in bits 3:0 and 15:14, expcnt in
    // 6:4, lgkmcnt in 11:8; another family needs another number)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // s_waitcnt vmcnt(0), expcnt and lgkmcnt left alone
    __syncthreads();
    if (t == 0) {
        __threadfence();
        red[3] = atomicAdd(&hy.ctl[HY_CTL_TICKET], 1u) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (red[3] == 0u) return;
    __threadfence();
    // (agent-scope loads: other CUs wrote these counts with atomics)
    uint32_t s4[4], m = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        s4[q] = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t c = ld_agent(&hy.top14[16u * t + 4u * q + j]);
            s4[q] += c;
            m = max(m, c);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor(m, off));
    if (lane == 0) atomicMax(&red[2], m);
    __syncthreads();
    const uint32_t diff = ~ld_agent(&hy.ctl[HY_CTL_NAND]) ^ ld_agent(&hy.ctl[HY_CTL_OR]);  // bits the keys differ in
    // k_plan8's rule, on the same numbers
    const bool hybrid = (diff & 255u) != 0u && ((diff >> 8) & 255u) != 0u && red[2] <= min(hy.limit, HY_MAX_BUCKET);
    if (t == 0) hy.ctl[HY_CTL_VERDICT] = hybrid ? HY_VERDICT_HYBRID : HY_VERDICT_CLASSIC;
    if (!hybrid) return;  // the full count follows and writes every field itself
    // What k_plan8 reads besides hps2 and top14, in the form k_hist_seg leaves it: the third joint
    // field (f = key >> 20, the sum of four top14 counts) and the digit-2 totals, as the marginal
    // of the second joint field with everything in nibble 0.  Digit 3's totals are the third
    // field's marginal; digits 0 and 1 stay zero, which is "not constant" (n > 0).
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t f = 4u * t + q;
        joint[(3u * NSEG + (f & 15u)) * 256 + (f >> 4)] = s4[q];
    }
    if (t < 256u) {
        uint32_t tot = 0;
        for (int s = 0; s < NSEG; ++s) tot += ld_agent(&hy.hps2[s * 256 + t]);
        joint[(2u * NSEG) * 256 + t] = tot;
    }
}

hipError_t launch_hist_lean(const uint32_t *keys, size_t n, uint32_t flip, uint32_t *joint, hipStream_t s,
                            const HyCounts &hy) {
    if (n == 0) return hipSuccess;
    HyCounts h = hy;
    if (n < HY_SAMPLE && h.mode == HY_COUNT_AUTO) h.mode = HY_COUNT_LEAN;  // too few keys to sample
    const uint32_t bps = hist_seg_bps(n);
    k_hist_lean<HY_LEAN_SL><<<NSEG * bps, HIST_BLOCK, 0, s>>>(keys, n, flip, joint, bps, h);
    return hipGetLastError();
}

}  // namespace labsort
