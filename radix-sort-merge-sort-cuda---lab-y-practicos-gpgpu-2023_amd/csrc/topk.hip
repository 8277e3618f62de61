// topk.hip -- top-k selection: the k smallest or largest keys of every row, with their positions
// (labsort_topk_device).  All kernels work on u, where plain uint32 order is the order asked for,
// formed where the raw input is read (tk_u) and undone where the keys are written (k_tk_write):
//   int32 / uint32   u = key ^ xr
//   float32          u = f32_ord(key) ^ xr
//   bfloat16/float16 u = (ord16(key) << 16) ^ xr, xr = largest ? 0xFFFF0000 : 0; the input is 2-byte
//                    elements, and two digit levels decide the threshold
// Every kernel that reads keys is written once and instantiated on the key type (TkKey): it says how a
// group of the raw input is loaded (quads of 32-bit words, octs of 16-bit elements that are widened)
// and mapped.  Everything behind the input reads (candidate buffer, survivor list, the inner sorts)
// holds 32-bit u for every key type.
//
// Rows longer than the segmented sort's pair tile are selected by an MSD radix select with 8-bit
// digits.  A row is cut into chunks of TK_CHUNK keys; per level:
//   k_tk_hist     counts the level's digit of the keys that match the prefix chosen so far: per
//                 chunk (cnt) and per row (hist)
//   k_tk_reduce   one wave per chunk: picks the digit d at which the row's running count reaches
//                 the remaining k, and sums the chunk's counts below d (low, accumulated over the
//                 levels) and at d (eq)
//   k_tk_scan     one workgroup per row: exclusive scans of low and eq over the chunks, the next
//                 level's state, and whether the row narrows
//   k_tk_compact  <false>, every level but the last, rows that narrow: one ordered pass over the
//                 input writes the keys below the bucket to the survivor list and the bucket to the
//                 candidate buffer; <true>, after the last level (3; 1 for 16-bit keys): the keys
//                 below the threshold and the first krem keys equal to it go to the survivor list
// Chunks are contiguous and every compaction places a chunk's keys at the chunk's scanned base in
// thread order, so keys of one value reach the survivor list in position order: the stable sort
// of the survivors that follows gives the tie rule for nothing.
// Every dependency is a kernel boundary; a workgroup beyond a row's current source returns at once.
#include "topk.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "devutil.h"
#include "host.h"
#include "segsort.h"

namespace labsort {

// Per row and level: what the level's kernels read.  Level L's scan writes entry L + 1, so no
// kernel reads a word that another workgroup of the same launch writes.
struct TkState {
    uint32_t prefix;    // digits chosen so far, in place (the top 8 * level bits)
    uint32_t krem;      // keys still to take among those that match the prefix (>= 1)
    uint32_t narrowed;  // 1: the source is the candidate buffer
    uint32_t ccount;    // pairs in the candidate buffer
    uint32_t sbase;     // survivors written so far (by the narrowing pass)
    uint32_t jn;        // 1: the previous level narrowed this row (its narrowing pass runs, low[] restarts)
    uint32_t tlow;      // keys of the source below the prefix: the sum of low[] after this level
    uint32_t pad;
};

struct TkArgs {
    const uint32_t *keys;                    // rows x cols, as the caller gave them (16-bit key types: 2-byte elements)
    uint32_t *hist;                          // [rows][TK_LEVELS][256]
    uint32_t *cnt;                           // [rows][nch][256]: each chunk's counts of the current level
    uint32_t *low, *eq, *lowbase, *eqbase;   // [rows][nch]: keys below the prefix / in the bucket, and their exclusive scans
    TkState *st;                             // [rows][TK_LEVELS + 1]
    uint32_t *cand_u, *cand_p;               // [rows][capa]
    uint32_t *surv_u, *surv_p;               // [rows][k]
    uint32_t cols, k, nch, capa, cap, xr;    // capa: cap rounded up to 64 words; xr: u = key ^ xr
};

namespace {

// What the raw input holds: the launchers pick the kernels by it.
enum TkKey : int { TK_INT, TK_F32, TK_BF16, TK_F16 };
constexpr bool tk_is16(int kt) { return kt == TK_BF16 || kt == TK_F16; }
constexpr uint32_t tk_nan_t(int kt) { return kt == TK_BF16 ? BF16_NAN_T : F16_NAN_T; }

struct TkSrc {
    // p == nullptr: the input (position = index, u = word ^ xr).  Of a 16-bit input only count
    // and xr are used: its elements are addressed through tk_raw16
    const uint32_t *u, *p;
    uint32_t count, xr;
};

__device__ __forceinline__ TkState tk_state(const TkArgs &a, uint32_t row, int level) {
    if (level == 0) return TkState{0u, a.k, 0u, 0u, 0u, 0u, 0u, 0u};
    return a.st[(size_t)row * (TK_LEVELS + 1) + level];
}

__device__ __forceinline__ TkSrc tk_src(const TkArgs &a, uint32_t row, const TkState &st) {
    if (st.narrowed) {
        const uint32_t c = st.ccount < a.cap ? st.ccount : a.cap;
        return TkSrc{a.cand_u + (size_t)row * a.capa, a.cand_p + (size_t)row * a.capa, c, 0u};
    }
    return TkSrc{a.keys + (size_t)row * a.cols, nullptr, a.cols, a.xr};
}

// Elements [beg, end) of a source are read in 16-byte aligned groups (devutil.h, load_group):
// quads of 32-bit words, or octs of a raw input of 16-bit elements.  Either way a key becomes u.
// tk_word: a word of the raw input of a float32 call (raw, uniform over the row) becomes its order
// image first; the candidate buffer already holds u.
template <int KT>
__device__ __forceinline__ uint32_t tk_word(uint32_t w, bool raw) {
    if constexpr (KT == TK_F32) return raw ? f32_ord(w) : w;
    else return w;
}
// u of an element x of the raw input: key ^ xr, f32_ord(key) ^ xr, or (ord16(key) << 16) ^ xr (ord16
// reads the low half of x)
template <int KT>
__device__ __forceinline__ uint32_t tk_u(uint32_t x, uint32_t xr) {
    if constexpr (tk_is16(KT)) return (ord16(x, tk_nan_t(KT)) << 16) ^ xr;
    else return tk_word<KT>(x, true) ^ xr;
}
template <int KT>
using tk_elem_t = std::conditional_t<tk_is16(KT), uint16_t, uint32_t>;
__device__ __forceinline__ const uint16_t *tk_raw16(const TkArgs &a, uint32_t row) {
    return reinterpret_cast<const uint16_t *>(a.keys) + (size_t)row * a.cols;
}
// Group q of the chunk [beg, end) of s as u[E], E keys per load: E = 8, octs of the raw 16-bit input
// (raw16); E = 4, quads of s.u, the raw input of a 32-bit call or a candidate buffer.  Returns the
// mask of the keys that exist; mis is the chunk's misalignment in that source.
template <int E, int KT>
__device__ __forceinline__ uint32_t tk_load(const TkSrc &s, const uint16_t *raw16, uint32_t beg, uint32_t end, uint32_t mis,
                                            uint32_t q, uint32_t (&u)[E], int64_t &i0) {
    static_assert(E == 4 || tk_is16(KT), "octs are a 16-bit call's reads of its raw input");
    const uint32_t xr = s.xr;
    if constexpr (E == 8) {
        return load_group(raw16, beg, end, mis, q, u, i0, [xr](uint32_t x) { return tk_u<KT>(x, xr); });
    } else {
        const bool raw = s.p == nullptr;
        return load_group(s.u, beg, end, mis, q, u, i0, [xr, raw](uint32_t w) { return tk_word<KT>(w, raw) ^ xr; });
    }
}

// The digit at which the running count of a row's level histogram reaches krem: the d with
// count(< d) < krem <= count(<= d).  Called by a whole wave; the result is wave-uniform.
struct TkPick {
    uint32_t d, below, bucket;
};
__device__ __forceinline__ TkPick tk_pick(const uint32_t *hrow, uint32_t krem, uint32_t lane) {
    const uint4 v = reinterpret_cast<const uint4 *>(hrow)[lane];  // digits 4 lane .. 4 lane + 3
    const uint32_t c[4] = {v.x, v.y, v.z, v.w};
    const uint32_t s = v.x + v.y + v.z + v.w;
    const uint32_t x = wave_incl_scan(s, lane);
    uint32_t run = x - s, d = 255u, below = x - c[3], bucket = c[3];  // (lane 63's default: the last digit)
    bool found = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!found && run < krem && krem <= run + c[j]) {
            found = true;
            d = 4u * lane + (uint32_t)j;
            below = run;
            bucket = c[j];
        }
        run += c[j];
    }
    const uint64_t m = __ballot(found);
    const int srcl = m ? __ffsll((long long)m) - 1 : 63;  // (no lane: krem exceeds the row's count, which cannot happen)
    TkPick p;
    p.d = __shfl(d, srcl);
    p.below = __shfl(below, srcl);
    p.bucket = __shfl(bucket, srcl);
    if (p.below >= krem) p.below = krem - 1u;  // keeps krem >= 1 whatever the histogram held
    return p;
}

// Counts into h (LDS) the level's digit of the keys of [beg, end) that match the prefix, E keys per
// load (tk_load); either way a thread has 16 keys in flight.
template <int E, int KT>
__device__ __forceinline__ void tk_hist_chunk(uint32_t *h, const TkSrc &s, const uint16_t *raw16, uint32_t beg, uint32_t end,
                                              uint32_t prefix, uint32_t mask, uint32_t shift, uint32_t tid) {
    constexpr int T = 16 / E;
    const uint32_t mis = E == 8 ? group_mis(raw16, beg) : group_mis(s.u, beg), nq = group_count<E>(beg, end, mis);
    for (uint32_t q0 = 0; q0 < nq; q0 += (uint32_t)T * TK_BLOCK) {
        uint32_t u[T][E], vm[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t q = q0 + (uint32_t)t * TK_BLOCK + tid;
            int64_t i0;
            vm[t] = q < nq ? tk_load<E, KT>(s, raw16, beg, end, mis, q, u[t], i0) : 0u;
        }
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int j = 0; j < E; ++j)
                if (((vm[t] >> j) & 1u) && ((u[t][j] ^ prefix) & mask) == 0u)
                    slot_hist_add<TK_SLOTS>(h, (u[t][j] >> shift) & 255u, tid);
    }
}

// One kernel for every key type KT.  A 16-bit call reads a row that has not narrowed from the raw
// input, eight keys per load, and a narrowed one from its candidate buffer of 32-bit u; a 32-bit
// call reads quads of either.
template <int KT>
__global__ __launch_bounds__(TK_BLOCK) void k_tk_hist(TkArgs a, int level, uint32_t nx, uint32_t g) {
    __shared__ uint32_t h[256 * TK_SLOTS];
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / nx, bx = blockIdx.x - row * nx;
    const TkState st = tk_state(a, row, level);
    const TkSrc s = tk_src(a, row, st);
    const uint16_t *raw16 = tk_raw16(a, row);
    const uint32_t nact = (s.count + TK_CHUNK - 1u) / TK_CHUNK;
    const uint32_t c0 = bx * g;
    if (c0 >= nact) return;
    const uint32_t c1 = c0 + g < nact ? c0 + g : nact;
    const uint32_t shift = 24u - 8u * (uint32_t)level;
    const uint32_t mask = level ? 0xFFFFFFFFu << (shift + 8u) : 0u;
    uint32_t acc = 0u;
    for (uint32_t c = c0; c < c1; ++c) {
        slot_hist_clear<TK_SLOTS, TK_BLOCK>(h, tid);
        __syncthreads();
        const uint32_t beg = c * TK_CHUNK, end = beg + TK_CHUNK < s.count ? beg + TK_CHUNK : s.count;
        if constexpr (tk_is16(KT)) {
            if (s.p == nullptr) tk_hist_chunk<8, KT>(h, s, raw16, beg, end, st.prefix, mask, shift, tid);  // (uniform over the workgroup)
            else tk_hist_chunk<4, KT>(h, s, raw16, beg, end, st.prefix, mask, shift, tid);
        } else {
            tk_hist_chunk<4, KT>(h, s, raw16, beg, end, st.prefix, mask, shift, tid);
        }
        __syncthreads();
        if (tid < 256u) {
            const uint32_t sum = slot_hist_fold<TK_SLOTS>(h, tid);
            a.cnt[((size_t)row * a.nch + c) * 256u + tid] = sum;
            acc += sum;
        }
        __syncthreads();
    }
    if (tid < 256u && acc) atomicAdd(&a.hist[((size_t)row * TK_LEVELS + level) * 256u + tid], acc);
}

constexpr int TK_RED_WAVES = 4;

__global__ __launch_bounds__(TK_RED_WAVES * WAVE) void k_tk_reduce(TkArgs a, int level, uint32_t nx) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t row = blockIdx.x / nx, bx = blockIdx.x - row * nx;
    const uint32_t chunk = bx * TK_RED_WAVES + wid;
    const TkState st = tk_state(a, row, level);
    const TkSrc s = tk_src(a, row, st);
    const uint32_t nact = (s.count + TK_CHUNK - 1u) / TK_CHUNK;
    if (chunk >= nact) return;  // (wave-uniform)
    const TkPick p = tk_pick(a.hist + ((size_t)row * TK_LEVELS + level) * 256u, st.krem, lane);
    const size_t idx = (size_t)row * a.nch + chunk;
    const uint4 v = reinterpret_cast<const uint4 *>(a.cnt + idx * 256u)[lane];
    const uint32_t c[4] = {v.x, v.y, v.z, v.w};
    uint32_t lo = 0u, e = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t dg = 4u * lane + (uint32_t)j;
        lo += dg < p.d ? c[j] : 0u;
        e += dg == p.d ? c[j] : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo += __shfl_xor(lo, off);
        e += __shfl_xor(e, off);
    }
    if (lane == 0u) {
        a.low[idx] = (level == 0 || st.jn) ? lo : a.low[idx] + lo;
        a.eq[idx] = e;
    }
}

// NLEV: the call's digit levels (4; 2 for 16-bit keys): no row narrows after the last one
template <int NLEV>
__global__ __launch_bounds__(TK_BLOCK) void k_tk_scan(TkArgs a, int level) {
    __shared__ uint32_t wsum[TK_BLOCK / WAVE], tot[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, row = blockIdx.x;
    const TkState st = tk_state(a, row, level);
    const TkSrc s = tk_src(a, row, st);
    const uint32_t nact = (s.count + TK_CHUNK - 1u) / TK_CHUNK;
    const TkPick p = tk_pick(a.hist + ((size_t)row * TK_LEVELS + level) * 256u, st.krem, lane);
    uint32_t carry_lo = 0u, carry_eq = 0u;
    for (uint32_t b = 0; b < nact; b += TK_BLOCK) {
        const uint32_t c = b + tid;
        const size_t idx = (size_t)row * a.nch + c;
        const uint32_t lo = c < nact ? a.low[idx] : 0u, e = c < nact ? a.eq[idx] : 0u;
        const uint32_t xl = block_excl_scan<TK_BLOCK, TK_BLOCK>(lo, wsum);
        __syncthreads();
        const uint32_t xe = block_excl_scan<TK_BLOCK, TK_BLOCK>(e, wsum);
        if (c < nact) {
            a.lowbase[idx] = carry_lo + xl;
            a.eqbase[idx] = carry_eq + xe;
        }
        if (tid == TK_BLOCK - 1u) {
            tot[0] = xl + lo;
            tot[1] = xe + e;
        }
        __syncthreads();
        carry_lo += tot[0];
        carry_eq += tot[1];
        __syncthreads();
    }
    if (tid == 0u) {
        const bool narrow = !st.narrowed && level < NLEV - 1 && p.bucket <= a.cap;
        TkState ns;
        ns.prefix = st.prefix | (p.d << (24u - 8u * (uint32_t)level));
        ns.krem = st.krem - p.below;
        ns.narrowed = (st.narrowed || narrow) ? 1u : 0u;
        ns.ccount = narrow ? p.bucket : st.ccount;
        ns.sbase = narrow ? carry_lo : st.sbase;
        ns.jn = narrow ? 1u : 0u;
        ns.tlow = carry_lo;
        ns.pad = 0u;
        a.st[(size_t)row * (TK_LEVELS + 1) + level + 1] = ns;
    }
}

// One ordered pass over a chunk.  FINAL = false (after level `level`, rows with jn set): the keys
// whose top digits lie below the new prefix go to the survivor list, those that match it to the
// candidate buffer.  FINAL = true: the keys below the threshold and the first krem keys equal to
// it go to the survivor list.  Every store is bounds-checked against its list.
// The pass is written once for E keys per thread and batch (ec): for a 16-bit call octs of the raw
// input (every narrowing pass, and the final one of a row that never narrowed) or quads of the
// candidate buffer, for a 32-bit call quads of either.
template <bool FINAL, int KT>
__global__ __launch_bounds__(TK_BLOCK) void k_tk_compact(TkArgs a, int level) {
    __shared__ uint32_t wsum[TK_BLOCK / WAVE], tot;
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / a.nch, chunk = blockIdx.x - row * a.nch;
    const TkState ns = a.st[(size_t)row * (TK_LEVELS + 1) + level + 1];
    if (!FINAL && !ns.jn) return;
    TkState from = ns;
    if (!FINAL) from.narrowed = 0u;  // a row narrows once, from the input
    const TkSrc s = tk_src(a, row, from);
    const uint32_t nact = (s.count + TK_CHUNK - 1u) / TK_CHUNK;
    if (chunk >= nact) return;
    const size_t idx = (size_t)row * a.nch + chunk;
    const uint32_t eqb = a.eqbase[idx];
    // (FINAL: nothing of this chunk is taken: no key below the threshold, its equals past the last one taken)
    if (FINAL && a.low[idx] == 0u && eqb >= ns.krem) return;
    const uint32_t lob = a.lowbase[idx] + (FINAL ? ns.sbase : 0u);
    const uint32_t mask = FINAL ? 0xFFFFFFFFu : 0xFFFFFFFFu << (24u - 8u * (uint32_t)level);
    const uint32_t P = ns.prefix;
    uint32_t *su = a.surv_u + (size_t)row * a.k, *sp = a.surv_p + (size_t)row * a.k;
    uint32_t *cu = a.cand_u + (size_t)row * a.capa, *cp = a.cand_p + (size_t)row * a.capa;
    const uint32_t beg = chunk * TK_CHUNK, end = beg + TK_CHUNK < s.count ? beg + TK_CHUNK : s.count;
    const uint16_t *raw16 = tk_raw16(a, row);
    auto pass = [&](auto ec) {
        constexpr int E = decltype(ec)::value;
        // one scan for both counts, 16 bits each: a batch holds at most 8192 keys
        static_assert(E * TK_BLOCK <= 65535, "the packed scan holds two 16-bit counts per batch");
        const uint32_t mis = E == 8 ? group_mis(raw16, beg) : group_mis(s.u, beg), nq = group_count<E>(beg, end, mis);
        uint32_t carry_l = 0u, carry_e = 0u;
        for (uint32_t q0 = 0; q0 < nq; q0 += TK_BLOCK) {
            const uint32_t q = q0 + tid;
            uint32_t u[E], pos[E], vm = 0u;
            int64_t i0 = 0;
            if (q < nq) vm = tk_load<E, KT>(s, raw16, beg, end, mis, q, u, i0);
#pragma unroll
            for (int j = 0; j < E; ++j) pos[j] = (uint32_t)(i0 + j);
            if constexpr (E == 4) {
                if (s.p) {
                    if (vm == 15u) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(s.p + i0);
                        pos[0] = v.x; pos[1] = v.y; pos[2] = v.z; pos[3] = v.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if ((vm >> j) & 1u) pos[j] = s.p[i0 + j];
                    }
                }
            }
            uint32_t lm = 0u, em = 0u;
#pragma unroll
            for (int j = 0; j < E; ++j)
                if ((vm >> j) & 1u) {
                    const uint32_t t = u[j] & mask;
                    lm |= (t < P ? 1u : 0u) << j;
                    em |= (t == P ? 1u : 0u) << j;
                }
            const uint32_t packed = (uint32_t)__popc(lm) | ((uint32_t)__popc(em) << 16);
            const uint32_t ex = block_excl_scan<TK_BLOCK, TK_BLOCK>(packed, wsum);
            if (tid == TK_BLOCK - 1u) tot = ex + packed;
            __syncthreads();
            uint32_t l = lob + carry_l + (ex & 0xFFFFu), e = eqb + carry_e + (ex >> 16);
            carry_l += tot & 0xFFFFu;
            carry_e += tot >> 16;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                if ((lm >> j) & 1u) {
                    if (l < a.k) {
                        su[l] = u[j];
                        sp[l] = pos[j];
                    }
                    ++l;
                }
                if ((em >> j) & 1u) {
                    if (FINAL) {
                        const uint32_t t = ns.sbase + ns.tlow + e;
                        if (e < ns.krem && t < a.k) {
                            su[t] = u[j];
                            sp[t] = pos[j];
                        }
                    } else if (e < a.cap) {
                        cu[e] = u[j];
                        cp[e] = pos[j];
                    }
                    ++e;
                }
            }
            __syncthreads();  // wsum and tot are reused by the next batch
        }
    };
    if constexpr (tk_is16(KT)) {
        if (!FINAL || s.p == nullptr) pass(std::integral_constant<int, 8>{});  // (uniform over the workgroup)
        else pass(std::integral_constant<int, 4>{});
    } else {
        pass(std::integral_constant<int, 4>{});
    }
}

// u[i] = tk_u of element i of the raw input, pos[i] = i % cols: for the paths that sort whole rows
// (one key per thread and load).  A 32-bit call may pass u == nullptr (the short path sorts the keys
// themselves); a 16-bit call always widens, and its loop stays free of the test.
template <int KT>
__global__ __launch_bounds__(256) void k_tk_prep(const tk_elem_t<KT> *__restrict__ keys, uint32_t *__restrict__ u,
                                                 uint32_t *__restrict__ pos, size_t n, uint32_t cols, uint32_t xr) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (tk_is16(KT) || u) u[i] = tk_u<KT>(keys[i], xr);
        pos[i] = (uint32_t)i % cols;  // (n <= 2^31 - 1)
    }
}

__global__ __launch_bounds__(256) void k_tk_offsets(uint32_t *__restrict__ off, uint32_t rows, uint32_t m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i <= rows; i += stride) off[i] = (uint32_t)i * m;
}

__global__ void k_tk_err_acc(uint32_t *hdr, const uint32_t *inner, int nw) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        uint32_t e = 0u;
        for (int i = 0; i < nw; ++i) e |= inner[i];
        if (e) hdr[0] = 1u;
    }
}

// grid: x over the k outputs of a row, rows folded into x as well (row = block / bpr).  The inverse
// of tk_u; a 16-bit call writes 2-byte elements (either format: unord16 is the same for both)
template <int KT>
__global__ __launch_bounds__(256) void k_tk_write(const uint32_t *__restrict__ su, const uint32_t *__restrict__ sp,
                                                  tk_elem_t<KT> *__restrict__ ko, uint32_t *__restrict__ io, uint32_t m,
                                                  uint32_t k, uint32_t bpr, uint32_t xr) {
    const uint32_t row = blockIdx.x / bpr, bx = blockIdx.x - row * bpr;
    const size_t src = (size_t)row * m, dst = (size_t)row * k;
    for (uint32_t j = bx * 256u + threadIdx.x; j < k; j += bpr * 256u) {
        const uint32_t w = su[src + j] ^ xr;
        if constexpr (tk_is16(KT)) ko[dst + j] = (uint16_t)unord16(w >> 16);
        else if constexpr (KT == TK_F32) ko[dst + j] = f32_unord(w);
        else ko[dst + j] = w;
        if (io) io[dst + j] = sp[src + j];
    }
}

unsigned tk_stream_blocks(size_t n) {
    const size_t b = (n + 256 * 8 - 1) / (256 * 8);
    return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

// kt: TkKey, the instantiation that runs.
hipError_t launch_topk_hist(const TkArgs &a, size_t rows, int level, int kt, hipStream_t s) {
    const uint32_t g = (a.nch + TK_MAX_HIST_WG - 1u) / TK_MAX_HIST_WG;  // chunks per workgroup
    const uint32_t nx = (a.nch + g - 1u) / g;
    const unsigned grid = (unsigned)(rows * nx);
    if (kt == TK_BF16) k_tk_hist<TK_BF16><<<grid, TK_BLOCK, 0, s>>>(a, level, nx, g);
    else if (kt == TK_F16) k_tk_hist<TK_F16><<<grid, TK_BLOCK, 0, s>>>(a, level, nx, g);
    else if (kt == TK_F32) k_tk_hist<TK_F32><<<grid, TK_BLOCK, 0, s>>>(a, level, nx, g);
    else k_tk_hist<TK_INT><<<grid, TK_BLOCK, 0, s>>>(a, level, nx, g);
    return hipGetLastError();
}

hipError_t launch_topk_reduce(const TkArgs &a, size_t rows, int level, hipStream_t s) {
    const uint32_t nx = (a.nch + TK_RED_WAVES - 1u) / TK_RED_WAVES;
    k_tk_reduce<<<(unsigned)(rows * nx), TK_RED_WAVES * WAVE, 0, s>>>(a, level, nx);
    return hipGetLastError();
}

// the digit levels of a call: two decide a 16-bit key
constexpr int TK_LEVELS16 = 2;
int tk_levels(int kt) { return tk_is16(kt) ? TK_LEVELS16 : TK_LEVELS; }

hipError_t launch_topk_scan(const TkArgs &a, size_t rows, int level, int kt, hipStream_t s) {
    if (tk_is16(kt)) k_tk_scan<TK_LEVELS16><<<(unsigned)rows, TK_BLOCK, 0, s>>>(a, level);
    else k_tk_scan<TK_LEVELS><<<(unsigned)rows, TK_BLOCK, 0, s>>>(a, level);
    return hipGetLastError();
}

template <bool FINAL>
hipError_t launch_topk_compact(const TkArgs &a, size_t rows, int level, int kt, hipStream_t s) {
    const unsigned grid = (unsigned)(rows * a.nch);
    if (kt == TK_BF16) k_tk_compact<FINAL, TK_BF16><<<grid, TK_BLOCK, 0, s>>>(a, level);
    else if (kt == TK_F16) k_tk_compact<FINAL, TK_F16><<<grid, TK_BLOCK, 0, s>>>(a, level);
    else if (kt == TK_F32) k_tk_compact<FINAL, TK_F32><<<grid, TK_BLOCK, 0, s>>>(a, level);
    else k_tk_compact<FINAL, TK_INT><<<grid, TK_BLOCK, 0, s>>>(a, level);
    return hipGetLastError();
}
hipError_t launch_topk_narrow(const TkArgs &a, size_t rows, int level, int kt, hipStream_t s) {
    return launch_topk_compact<false>(a, rows, level, kt, s);
}
hipError_t launch_topk_final(const TkArgs &a, size_t rows, int kt, hipStream_t s) {
    return launch_topk_compact<true>(a, rows, tk_levels(kt) - 1, kt, s);
}

// u[i] = keys[i] ^ xr (TK_F32: f32_ord(keys[i]) ^ xr; 16-bit kinds: (ord16(keys[i]) << 16) ^ xr, keys
// 2-byte elements; u may be nullptr), pos[i] = i % cols
hipError_t launch_topk_prep(const void *keys, uint32_t *u, uint32_t *pos, size_t n, size_t cols, uint32_t xr, int kt,
                            hipStream_t s) {
    const unsigned grid = tk_stream_blocks(n);
    const uint32_t *k32 = static_cast<const uint32_t *>(keys);
    const uint16_t *k16 = static_cast<const uint16_t *>(keys);
    if (kt == TK_BF16) k_tk_prep<TK_BF16><<<grid, 256, 0, s>>>(k16, u, pos, n, (uint32_t)cols, xr);
    else if (kt == TK_F16) k_tk_prep<TK_F16><<<grid, 256, 0, s>>>(k16, u, pos, n, (uint32_t)cols, xr);
    else if (kt == TK_F32) k_tk_prep<TK_F32><<<grid, 256, 0, s>>>(k32, u, pos, n, (uint32_t)cols, xr);
    else k_tk_prep<TK_INT><<<grid, 256, 0, s>>>(k32, u, pos, n, (uint32_t)cols, xr);
    return hipGetLastError();
}

// off[i] = i * m, i <= rows
hipError_t launch_topk_offsets(uint32_t *off, size_t rows, size_t m, hipStream_t s) {
    k_tk_offsets<<<tk_stream_blocks(rows + 1), 256, 0, s>>>(off, (uint32_t)rows, (uint32_t)m);
    return hipGetLastError();
}

// hdr[0] |= any of inner[0 .. nw) set
hipError_t launch_topk_err_acc(uint32_t *hdr, const uint32_t *inner, int nw, hipStream_t s) {
    k_tk_err_acc<<<1, 64, 0, s>>>(hdr, inner, nw);
    return hipGetLastError();
}

// keys_out[r][j] = su[r * m + j] ^ xr (f32: f32_unord of it; 16-bit keys: unord16 of its top half, a
// 2-byte element), idx_out[r][j] = sp[r * m + j] for j < k (idx_out may be nullptr)
hipError_t launch_topk_write(const uint32_t *su, const uint32_t *sp, void *keys_out, uint32_t *idx_out, size_t rows,
                             size_t m, size_t k, uint32_t xr, int kt, hipStream_t s) {
    // blocks per row: enough for one key per thread, fewer when there are many rows
    size_t bpr = (k + 255) / 256;
    const size_t room = ((size_t)1 << 20) / rows;
    if (bpr > room) bpr = room ? room : 1;
    const unsigned grid = (unsigned)(rows * bpr);
    uint32_t *ko = static_cast<uint32_t *>(keys_out);
    // (one 16-bit instantiation serves both formats)
    if (tk_is16(kt)) k_tk_write<TK_BF16><<<grid, 256, 0, s>>>(su, sp, static_cast<uint16_t *>(keys_out), idx_out, (uint32_t)m, (uint32_t)k, (uint32_t)bpr, xr);
    else if (kt == TK_F32) k_tk_write<TK_F32><<<grid, 256, 0, s>>>(su, sp, ko, idx_out, (uint32_t)m, (uint32_t)k, (uint32_t)bpr, xr);
    else k_tk_write<TK_INT><<<grid, 256, 0, s>>>(su, sp, ko, idx_out, (uint32_t)m, (uint32_t)k, (uint32_t)bpr, xr);
    return hipGetLastError();
}

}  // namespace

}  // namespace labsort

using namespace labsort;

extern "C" {

// ---------------------------------------------------------------------------------
// host driver and C-ABI: the k best keys of every row, sorted, with their positions
// ---------------------------------------------------------------------------------
namespace {
static_assert(TK_SORT_DIV == LABSORT_TOPK_SORT_DIV, "labsort.h states the large-k threshold");
static_assert(SEG_HDR_CNT * 4 + SEG_CLASSES * 4 <= TK_HDR_BYTES && TK_HDR_BYTES == SEG_HDR_BYTES,
              "the short path hands its header to the segmented sort's kernels");
enum { TK_PATH_SHORT, TK_PATH_SELECT, TK_PATH_SORT };

// Which path runs: host arguments only.  Whole-row sorting needs the inner sort's limits (one row:
// any length; several: the segmented sort's general path), else the select serves every k.
int topk_path(size_t rows, size_t cols, size_t k) {
    if (cols <= (size_t)SEG_TILE_PAIRS) return TK_PATH_SHORT;
    const bool sort_ok = rows == 1 || rows * cols <= RADIX_MAX_N;
    bool want_sort = k * (size_t)TK_SORT_DIV > cols;
    // LABSORT_TOPK_PATH=select / sort forces the long rows' path (harness/topk_bench.py --sweep)
    if (const char *e = std::getenv("LABSORT_TOPK_PATH")) {
        if (!std::strcmp(e, "select")) want_sort = false;
        else if (!std::strcmp(e, "sort")) want_sort = true;
    }
    return (want_sort && sort_ok) ? TK_PATH_SORT : TK_PATH_SELECT;
}

// header | (select: hist, state, per-chunk tables, candidate buffers) | A, B: the m (u, position)
// pairs per row to be ordered | SU, SP: the same, ordered | uniform offsets | the inner sort's
// workspace.  m = k after a select, cols where whole rows are sorted.  The short path keeps the
// segmented sort's class lists where the others keep the inner workspace, and has no A.
struct TopkLayout {
    int path;
    size_t m, nch, cap, capa;
    size_t off_hist, zero_bytes, off_st, off_cnt, off_low, off_eq, off_lowbase, off_eqbase, off_cand_u, off_cand_p;
    size_t off_a, off_b, off_su, off_sp, off_offs, off_lists, list_stride, off_inner, inner_bytes, total;
};
TopkLayout topk_layout_path(size_t rows, size_t cols, size_t k, int path) {
    TopkLayout L{};
    L.path = path;
    L.m = path == TK_PATH_SELECT ? k : cols;
    Carver c{TK_HDR_BYTES};
    if (path == TK_PATH_SELECT) {
        L.nch = (cols + TK_CHUNK - 1) / TK_CHUNK;
        L.cap = cols / TK_CAND_DIV;
        L.capa = align_up(L.cap, 64);
        L.off_hist = c.take(rows * TK_LEVELS * 256 * 4);
        L.zero_bytes = c.o;  // header and histograms: the only words a call relies on being clear
        L.off_st = c.take(rows * (TK_LEVELS + 1) * sizeof(TkState));
        L.off_cnt = c.take(rows * L.nch * 256 * 4);
        L.off_low = c.take(rows * L.nch * 4);
        L.off_eq = c.take(rows * L.nch * 4);
        L.off_lowbase = c.take(rows * L.nch * 4);
        L.off_eqbase = c.take(rows * L.nch * 4);
        L.off_cand_u = c.take(rows * L.capa * 4);
        L.off_cand_p = c.take(rows * L.capa * 4);
    } else {
        L.zero_bytes = c.o;
    }
    const size_t n = rows * L.m;
    if (path != TK_PATH_SHORT) L.off_a = c.take(n * 4);
    L.off_b = c.take(n * 4);
    L.off_su = c.take(n * 4);
    L.off_sp = c.take(n * 4);
    L.off_offs = c.take((rows + 1) * 4);
    if (path == TK_PATH_SHORT) {
        L.list_stride = align_up(rows * 4, 256) / 4;
        L.off_lists = c.take((size_t)SEG_CLASSES * L.list_stride * 4);
    } else {
        L.inner_bytes = rows == 1 ? seg_inner_bytes(n) : labsort_segments_workspace_bytes(n, rows, L.m, 1);
        L.off_inner = c.take(L.inner_bytes);
    }
    L.total = c.o;
    return L;
}
TopkLayout topk_layout(size_t rows, size_t cols, size_t k) {
    const int path = topk_path(rows, cols, k);
    TopkLayout L = topk_layout_path(rows, cols, k, path);
    // never less than the largest select below the threshold: the size does not shrink as k grows
    if (path == TK_PATH_SORT && cols / TK_SORT_DIV >= 1)
        L.total = std::max(L.total, topk_layout_path(rows, cols, cols / TK_SORT_DIV, TK_PATH_SELECT).total);
    return L;
}
}  // namespace

size_t labsort_topk_workspace_bytes(size_t rows, size_t cols, size_t k) {
    if (rows == 0 || k == 0 || k > cols || rows > (size_t)0x7FFFFFFFu / cols) return TK_HDR_BYTES;
    return topk_layout(rows, cols, k).total;
}

int labsort_topk_device(const void *d_keys, size_t rows, size_t cols, size_t k, int largest, int key_type,
                        void *d_keys_out, uint32_t *d_idx_out, void *d_ws, size_t ws_bytes, void *stream) {
    if (rows == 0 || k == 0) return LABSORT_OK;
    if (!topk_key_type_ok(key_type)) return LABSORT_ERR_ARG;
    if (const int rc = dense_rows_args(d_keys, rows, cols, k, key_type, d_keys_out, d_idx_out)) return rc;
    const bool k16 = key_type_is16(key_type);
    const int path = topk_path(rows, cols, k);
    // the survivors of several long rows are ordered by the segmented sort: past its LDS tile, its general path
    if (path == TK_PATH_SELECT && rows > 1 && k > (size_t)SEG_TILE_PAIRS && rows * k > RADIX_MAX_N) return LABSORT_ERR_ARG;
    if (!d_ws || ws_bytes < labsort_topk_workspace_bytes(rows, cols, k)) return LABSORT_ERR_ARG;
    const TopkLayout L = topk_layout_path(rows, cols, k, path);
    // 16-bit keys: u = (ord16(key) << 16) ^ xr, its low half clear
    const uint32_t xr = k16 ? (largest ? 0xFFFF0000u : 0u) : flip_of(key_type) ^ (largest ? 0xFFFFFFFFu : 0u);
    const bool f32 = key_type == LABSORT_KEY_F32;  // u = f32_ord(key) ^ xr
    const int kt = f32 ? TK_F32 : key_type == LABSORT_KEY_BF16 ? TK_BF16 : key_type == LABSORT_KEY_F16 ? TK_F16 : TK_INT;
    hipStream_t s = as_stream(stream);
    char *ws = static_cast<char *>(d_ws);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t *>(ws + off); };
    const uint32_t *keys = static_cast<const uint32_t *>(d_keys);  // (a 16-bit call reads 2-byte elements: k_tk_prep, tk_raw16)
    uint32_t *hdr = W(0), *A = W(L.off_a), *B = W(L.off_b), *SU = W(L.off_su), *SP = W(L.off_sp), *offs = W(L.off_offs);
    void *ko = d_keys_out;
    const size_t n = rows * L.m;
    HIP_TRY(launch_zero(ws, L.zero_bytes, s));  // (a kernel: graph-replayable)
    if (path == TK_PATH_SHORT) {
        // whole rows through the segmented sort's LDS classes, on (key, position) with xr as the flip
        TimingScope ts(LABSORT_K_TOPK, s);
        uint32_t *lists = W(L.off_lists);
        HIP_TRY(launch_topk_offsets(offs, rows, cols, s));
        // 16-bit keys: the class kernels load 32-bit words, so the keys are first widened to
        // ord16(key) << 16 into SU and sorted there in place (a class kernel holds its whole segment in
        // registers before its first store, as the in-place segmented sort relies on)
        if (k16) HIP_TRY(launch_topk_prep(keys, SU, B, n, cols, 0u, kt, s));
        else HIP_TRY(launch_topk_prep(keys, nullptr, B, n, cols, xr, TK_INT, s));  // (positions only)
        HIP_TRY(launch_seg_bin(offs, rows, n, cols, true, true, hdr, lists, L.list_stride, s));
        HIP_TRY(launch_seg_lds_classes(cols, true, k16 ? SU : keys, SU, B, SP, offs, hdr, lists, L.list_stride, xr, f32, s));
        // (the class kernels wrote keys, not u: nothing to undo but, for 16-bit keys, ord16)
        HIP_TRY(launch_topk_write(SU, SP, ko, d_idx_out, rows, cols, k, 0u, k16 ? kt : TK_INT, s));
        return LABSORT_OK;
    }
    if (path == TK_PATH_SELECT) {
        TimingScope ts(LABSORT_K_TOPK, s);
        TkArgs a{};
        a.keys = keys;
        a.hist = W(L.off_hist);
        a.cnt = W(L.off_cnt);
        a.low = W(L.off_low);
        a.eq = W(L.off_eq);
        a.lowbase = W(L.off_lowbase);
        a.eqbase = W(L.off_eqbase);
        a.st = reinterpret_cast<TkState *>(ws + L.off_st);
        a.cand_u = W(L.off_cand_u);
        a.cand_p = W(L.off_cand_p);
        a.surv_u = A;
        a.surv_p = B;
        a.cols = (uint32_t)cols;
        a.k = (uint32_t)k;
        a.nch = (uint32_t)L.nch;
        a.capa = (uint32_t)L.capa;
        a.cap = (uint32_t)L.cap;
        a.xr = xr;
        const int nlev = tk_levels(kt);
        for (int level = 0; level < nlev; ++level) {
            HIP_TRY(launch_topk_hist(a, rows, level, kt, s));
            HIP_TRY(launch_topk_reduce(a, rows, level, s));
            HIP_TRY(launch_topk_scan(a, rows, level, kt, s));
            if (level < nlev - 1 && L.cap > 0) HIP_TRY(launch_topk_narrow(a, rows, level, kt, s));
        }
        HIP_TRY(launch_topk_final(a, rows, kt, s));
    } else {
        TimingScope ts(LABSORT_K_TOPK, s);
        HIP_TRY(launch_topk_prep(keys, A, B, n, cols, xr, kt, s));
    }
    // order the m pairs of every row on u (stable): one pair sort, or the segmented pair sort
    char *iws = ws + L.off_inner;
    uint32_t *ierr = reinterpret_cast<uint32_t *>(iws);
    HIP_TRY(launch_zero(ierr, 16, s));  // (a one-tile inner sort has no error word of its own)
    int st;
    if (rows == 1) {
        if ((st = labsort_sort_pairs_device(A, B, SU, SP, n, LABSORT_KEY_U32, LABSORT_ALGO_AUTO, iws, L.inner_bytes, stream)))
            return st;
    } else {
        {
            TimingScope ts(LABSORT_K_TOPK, s);
            HIP_TRY(launch_topk_offsets(offs, rows, L.m, s));
        }
        if ((st = labsort_sort_segments_pairs_device(A, B, SU, SP, n, offs, rows, L.m, LABSORT_KEY_U32, iws, L.inner_bytes,
                                                     stream)))
            return st;
    }
    TimingScope ts(LABSORT_K_TOPK, s);
    HIP_TRY(launch_topk_err_acc(hdr, ierr, 2, s));
    HIP_TRY(launch_topk_write(SU, SP, ko, d_idx_out, rows, L.m, k, xr, kt, s));
    return LABSORT_OK;
}

int labsort_topk_workspace_status(const void *d_ws, void *stream) {
    uint32_t w = 0;
    if (const int st = read_ws_words(d_ws, &w, 1, as_stream(stream))) return st;
    return w ? LABSORT_ERR_DEVICE : LABSORT_OK;
}

}  // extern "C"
