/*
 * include/labsort.h -- C-ABI of liblabsort.so, the MI355X-native (gfx950) sort.
 *
 * Plain pointers and sizes only (no HIP or torch types): `stream` is a
 * hipStream_t passed as void* (NULL = the null stream), device pointers come
 * from hipMalloc / torch tensors.  Every function returns a LABSORT_* status.
 *
 * What each entry replaces in the reference (`Sord Radix y Merge/`):
 *   labsort_sort_host      order_array(int*, int)               lab.cu:303-402, lab.h:9
 *                          (host pointer in, sorted in place, synchronous)
 *   labsort_sort_device    stages 1-3 of order_array between the H2D copy
 *                          (lab.cu:321) and the D2H copy (lab.cu:397)
 *   labsort_wave_tile_sort radix_sort_kernel (lab.cu:47-87): per-tile bit
 *                          split with early exit, wave64 tiles instead of warp32
 *   labsort_tile_sort      stage 1+2 of order_array (lab.cu:323-346): sorted
 *                          runs of labsort_tile_keys() keys
 *   labsort_merge_pass     stage 3 iteration (separators_kernel +
 *                          merge_segments_kernel, lab.cu:358-391)
 *   labsort_merge          deviceOrderedJoin (lab.cu:144-182) generalised to a
 *                          diagonal range of merge(A,B); used by the multi-GPU
 *                          merge-split exchange
 *   labsort_histogram      the global digit count of letra.pdf's split (no
 *                          counterpart kernel in lab.cu)
 *   sort(int*, int)        the north_star's name for order_array
 * The C++-linkage drop-ins order_array / order_with_trust live in lab.h.
 */
#ifndef LABSORT_H
#define LABSORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define LABSORT_OK 0
#define LABSORT_ERR_ARG 1        /* bad argument (NULL, n too large, workspace too small) */
#define LABSORT_ERR_HIP 2        /* a HIP runtime call failed: labsort_last_hip_error() */
#define LABSORT_ERR_DEVICE 3     /* a kernel reported an internal error (bounded spin expired) */
#define LABSORT_ERR_PEER 4       /* distributed sort: another rank failed (this one gave up with it) */

/* algorithms */
#define LABSORT_ALGO_RADIX 0     /* LSD radix, 8-bit digits: gathered passes for 2^16 <= n < 2^25,
                                    onesweep scatter passes outside (LABSORT_RADIX_IMPL=onesweep or
                                    =gather forces one) */
#define LABSORT_ALGO_MERGE 1     /* LDS tile radix + merge-path merge passes */
#define LABSORT_ALGO_RADIX1 2    /* LSD radix with 1-bit digits: letra.pdf's split, 32 passes */
#define LABSORT_ALGO_AUTO 3      /* MERGE for n <= LABSORT_AUTO_MERGE_MAX_KEYS (fewer launches and
                                    less fixed cost at small n) and above the radix limit
                                    (labsort_max_keys(RADIX), e.g. 2^30 keys), RADIX between; the
                                    default of the host drop-ins order_array / sort (LABSORT_ALGO
                                    env overrides) */
#define LABSORT_AUTO_MERGE_MAX_KEYS (1u << 16) /* r27: the fused gathered radix wins from ~1.5 x 2^16 */
/* key/value sorts (labsort_sort_pairs_device, AUTO): merge up to here.  Their radix has no
   fused small path (histogram, plan and four persistent passes at every size), so they keep
   the r19 crossover measured before the keys-only threshold moved */
#define LABSORT_AUTO_PAIRS_MERGE_MAX_KEYS (1u << 18)

/* key types: how the 32-bit words are ordered */
#define LABSORT_KEY_U32 0
#define LABSORT_KEY_I32 1
/* IEEE-754 binary32.  A word x is ordered by its image
 *   ord(x) = 0xFFFFFFFF        if x is a NaN ((x & 0x7FFFFFFF) > 0x7F800000)
 *          = ~x                if the sign bit is set
 *          = x | 0x80000000    otherwise
 * in plain uint32 order: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN.  -0.0 sorts before +0.0
 * (the two stay distinct words, so the result is deterministic); every NaN equals every other
 * and is greater than everything else, as in torch.sort / torch.topk.  Ties, NaNs included,
 * are broken by position wherever an entry promises stability or a tie order.  Non-NaN keys
 * come back bit-exact.  A NaN comes back as a NaN, its sign and payload not promised: paths
 * that sort the image write unord(0xFFFFFFFF) = 0x7FFFFFFF (labsort_sort_device,
 * labsort_sort_pairs_device, the segmented sorts' LDS path, top-k), paths that gather from the
 * input write the original word (the segmented sorts' general path in its pairs form), where
 *   unord(o) = (o & 0x80000000) ? (o & 0x7FFFFFFF) : ~o.
 * Accepted by labsort_sort_device, labsort_sort_pairs_device, labsort_sort_segments_device,
 * labsort_sort_segments_pairs_device, labsort_topk_device, labsort_sort_rows_device, labsort_kth_device and
 * labsort_unique_device, labsort_searchsorted_device and labsort_bucket_counts_device only; every other entry that
 * checks its key type returns LABSORT_ERR_ARG for it (labsort_bincount_device, host-pointer, multi-GPU and distributed
 * sorts, labsort_merge_runs, labsort_upper_bound, the C++ drop-ins).  The building blocks
 * that take a key type without checking it order U32 / I32 words only. */
#define LABSORT_KEY_F32 2
/* bfloat16 and IEEE-754 binary16: 16-bit elements, accepted by labsort_topk_device,
 * labsort_sort_rows_device, labsort_sort16_device, labsort_searchsorted_device and labsort_bucket_counts_device ONLY (every other entry that checks its key type returns
 * LABSORT_ERR_ARG for them, the segmented and whole-array device sorts included).  The float32 contract at 16 bits: with T = 0x7F80 (bfloat16)
 * or 0x7C00 (binary16), an element x is ordered by
 *   ord16(x) = 0xFFFF         if (x & 0x7FFF) > T   (every NaN, either sign)
 *            = ~x & 0xFFFF    if x & 0x8000
 *            = x | 0x8000     otherwise
 * so -inf < ... < -0.0 < +0.0 < ... < +inf < NaN, every NaN equal and last, ties (NaNs included)
 * by position; non-NaN keys come back bit-exact and a NaN as 0x7FFF, a NaN in both formats, by
 *   unord16(o) = (o & 0x8000) ? (o & 0x7FFF) : (~o & 0xFFFF). */
#define LABSORT_KEY_BF16 3
#define LABSORT_KEY_F16 4
/* The order image of a key word, and its inverse (host functions; the kernels compile the same
 * definition): U32 word, I32 word ^ 0x80000000, F32 ord(word) / unord(bits) as above; BF16 / F16
 * ord16 / unord16 of the argument's low 16 bits, a result in [0, 0xFFFF].  An unknown key type
 * gives the word back. */
uint32_t labsort_key_order_bits(uint32_t word, int key_type);
uint32_t labsort_key_from_order_bits(uint32_t bits, int key_type);
/* 8-byte keys: uint64, int64 and IEEE-754 binary64, accepted by labsort_sort64_device,
 * labsort_unique_device, labsort_searchsorted_device and labsort_bucket_counts_device ONLY, U64 and
 * I64 by labsort_bincount_device too (every
 * other entry that checks its key type returns LABSORT_ERR_ARG for them; values 5 to 7 are not
 * assigned).  The order image is a uint64_t: U64 the word, I64 the word ^ (1 << 63), F64 the
 * float32 contract at 64 bits,
 *   ord64(x) = ~0             if (x & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000   (every NaN, either sign)
 *            = ~x             if the sign bit is set
 *            = x | (1 << 63)  otherwise
 * so -inf < ... < -0.0 < +0.0 < ... < +inf < NaN, every NaN equal and last, ties (NaNs included)
 * by position; non-NaN keys come back bit-exact and a NaN as 0x7FFFFFFFFFFFFFFF, by
 *   unord64(o) = (o >> 63) ? (o & 0x7FFFFFFFFFFFFFFF) : ~o. */
#define LABSORT_KEY_U64 8
#define LABSORT_KEY_I64 9
#define LABSORT_KEY_F64 10
/* The 64-bit order image of an 8-byte key word and its inverse (host functions; the kernels compile
 * the same definition).  Another key type gives the word back, as the 32-bit pair above does for
 * these three. */
uint64_t labsort_key_order_bits64(uint64_t word, int key_type);
uint64_t labsort_key_from_order_bits64(uint64_t bits, int key_type);

/* generator distributions (oracle/cpu_sort.cpp uses the same codes and formula) */
#define LABSORT_DIST_U32 0
#define LABSORT_DIST_U31 1
#define LABSORT_DIST_MOD100 2
#define LABSORT_DIST_MOD1000 3
#define LABSORT_DIST_SORTED 4
#define LABSORT_DIST_REVERSED 5
#define LABSORT_DIST_CONST 6
#define LABSORT_DIST_LOWBITS 7

/* kernel classes for the timing hooks */
#define LABSORT_K_HISTOGRAM 0
#define LABSORT_K_ONESWEEP 1
#define LABSORT_K_TILE_SORT 2
#define LABSORT_K_MERGE 3
#define LABSORT_K_PARTITION 4
#define LABSORT_K_GSWEEP 5       /* gathered radix pass (LABSORT_ALGO_RADIX, 2^16 <= n < 2^25) */
#define LABSORT_K_GCOPY 6        /* its final gathered copy */
#define LABSORT_K_COPY 7         /* the streaming copy (labsort_copy: the bench's copy ceiling) */
#define LABSORT_K_MERGE4 8       /* four-way merge pass of the merge sort (k_m4_rank + k_m4_merge) */
#define LABSORT_K_SEGSORT 9      /* segmented sort: classification, the LDS class kernels, the general path's glue;
                                    also the hybrid radix sort's finish (bucket offsets, lists, class kernels) */
#define LABSORT_K_TOPK 10        /* top-k selection: the select's own kernels and the glue around the inner sorts */
#define LABSORT_K_COUNT 11

/* ---- library info ---- */
const char *labsort_version(void);
const char *labsort_error_string(int status);
int labsort_last_hip_error(void);                 /* hipError_t of the last failure */
const char *labsort_hip_error_string(int hip_error);
size_t labsort_max_keys(int algo);                /* largest n a device sort accepts */
size_t labsort_tile_keys(void);                   /* run length produced by labsort_tile_sort */
size_t labsort_merge_tile_keys(void);             /* output keys per merge workgroup */

/* ---- whole sorts ---- */
/* Bytes of device workspace labsort_sort_device needs for n keys. */
size_t labsort_workspace_bytes(size_t n, int algo);
/* Sort n keys from d_in into d_out (d_in == d_out allowed: in place).
 * Asynchronous on `stream`; no host synchronisation, graph-capturable.
 * key_type LABSORT_KEY_F32: one streaming kernel writes the order image of d_in into d_out, the
 * sort runs in place on it as LABSORT_KEY_U32 with the same algo and workspace, one streaming
 * kernel undoes the image in place: two more sweeps over the keys (about 0.37 ms each at 2^28).
 * d_in is not written when d_out differs; NaNs come back as 0x7FFFFFFF. */
int labsort_sort_device(const void *d_in, void *d_out, size_t n, int key_type, int algo, void *d_workspace,
                        size_t workspace_bytes, void *stream);
/* Host pointer in/out, synchronous: the order_array contract (lab.cu:303).
 * From 2^27 keys the copies are pipelined: 8 chunks copied H2D while earlier chunks
 * sort (each by `algo` resolved at the chunk's size), two half merges, and the final
 * merge by 8 diagonal ranges whose D2H copies start as each range lands
 * (LABSORT_HOST_PIPE=0 turns it off, =1 forces it from 2^16 keys).
 * Returns LABSORT_ERR_DEVICE when a kernel reported an internal error. */
int labsort_sort_host(void *h_keys, size_t n, int key_type, int algo);
/* Device-side status of the last labsort_sort_device(n, algo) that used d_workspace:
 * synchronises `stream`, then returns LABSORT_ERR_DEVICE if a kernel of that sort set
 * the workspace's error word (radix: a bounded look-back spin expired; merge: a four-way
 * block whose cuts were inconsistent was skipped -- the result is not valid), else
 * LABSORT_OK.  The error word is the first 32-bit word of the workspace, cleared at the
 * start of every sort longer than one tile (one tile: no error word, LABSORT_OK).  The
 * reference's policy (CUDA_CHK after every launch, utils.h:18-26) checks launch status
 * only; this adds the kernels' own failure report. */
int labsort_workspace_status(const void *d_workspace, size_t n, int algo, void *stream);
/* Which path the last keys-only LABSORT_ALGO_RADIX sort of n keys on d_workspace took, after
 * synchronising `stream`: 0 the classic four scatter passes (also: gathered passes, one tile,
 * key/value sorts), 1 the hybrid path -- scatter passes on the two high digits, then every
 * bucket of the top 16 bits sorted in LDS.  The choice is made on the device from the keys:
 * hybrid when both low digits vary and no value of the top 14 bits has more than 20480 keys.
 * LABSORT_RADIX_HYBRID (read per call): unset or =1 offers it for 15 * 2^24 <= n <= 19 * 2^24
 * keys, where it measured faster; =0 never; =2 at every n the onesweep passes take, and up to
 * 32768 keys per value of the top 14 bits, the bound that keeps it correct.  The workspace of
 * the onesweep passes holds the path's counters, bucket offsets and lists at every n.
 * A negative value: -LABSORT_ERR_HIP. */
int labsort_radix_path(const void *d_workspace, size_t n, void *stream);
/* Which upfront count the last keys-only LABSORT_ALGO_RADIX sort of n keys on d_workspace ran,
 * after synchronising `stream`: 0 the full count only (also: host gate closed, key/value sorts,
 * gathered passes, one tile, no workspace), 1 the hybrid path's lean count only (two counters per
 * key, the path decided by its last workgroup), 2 the lean count, whose verdict was "classic", and
 * then the full count.  With the host gate open a fixed sample of the keys chooses which count
 * runs first; the path taken never depends on that choice.  LABSORT_HY_COUNT (read per call):
 * unset or =auto the sample chooses, =lean the lean count always runs first, =full the full
 * count only.  A negative value: -LABSORT_ERR_HIP. */
int labsort_radix_counting(const void *d_workspace, size_t n, void *stream);
/* The same for the last labsort_sort_pairs_device(n, algo) on d_workspace. */
int labsort_pairs_workspace_status(const void *d_workspace, size_t n, int algo, void *stream);

/* ---- the merge-sort path across GPUs (the reference
 * is single-GPU, lab.cu:303-402).  One schedule (csrc/dist_plan.h) for every form:
 * each rank sorts its shard locally (LABSORT_ALGO_AUTO), the ranks agree on p-1
 * (key, rank, position) splitters from a regular sample of every sorted shard, cut
 * their shards at them (labsort_upper_bound), send piece j to rank j by pairwise
 * send/recv with every peer at once, and merge the p received runs in rank order
 * (labsort_merge_runs pair passes, then the last level by diagonal ranges).  Rank r
 * ends with the contiguous range [goff, goff + count) of the sorted array. ----
 *
 * One process, several GPUs (one host thread per rank): sort a host buffer in place.
 * Rank r copies the shard h_keys[r*n/p, (r+1)*n/p) over its own PCIe link in 8 chunks
 * while earlier chunks sort (from 2^24 keys per rank; LABSORT_HOST_PIPE=0 never, =1
 * from 2^16), and copies its merged range back to its global offset range by range as
 * the last merge level lands.  LABSORT_PIN=1 page-locks the caller's array for the
 * call (hipHostRegister).  transport: LABSORT_XFER_PEER (hipMemcpyPeerAsync into each
 * receiver's slot; ranks may share a device), LABSORT_XFER_RCCL (ncclSend/ncclRecv
 * with every peer in one group per rank, communicators from ncclCommInitAll; one rank
 * per device) or LABSORT_XFER_AUTO (= PEER).  Synchronous.  order_array / sort use
 * labsort_sort_host_multi when LABSORT_GPUS > 1. */
#define LABSORT_XFER_AUTO 0
#define LABSORT_XFER_RCCL 1
#define LABSORT_XFER_PEER 2
#define LABSORT_MULTI_MAX_RANKS 8
/* phases of labsort_multi_timing / labsort_dist_timing, ms of the last call (device
 * timeline, max over ranks; phases may overlap): 0 H2D (host input), 1 local sort,
 * 2 plan (samples + splitters + cut points, collectives included), 3 exchange, 4 merge,
 * 5 D2H tail after the merge (host output), 6 total (host wall time), 7 the plan's own
 * work (host clock: from the rank's local sort seen complete to the plan's end, minus
 * the time spent inside its collectives), 8 the plan's wait (time inside the
 * collectives: mostly waiting for the slowest rank to arrive) */
#define LABSORT_MULTI_PHASES 9
/* Collectives of one schedule call, in order: 0 samples (allgather), 1 piece counts
 * (allgather), 2 buffer growth (allgather; runs only when a range outgrew the pre-sized
 * receive buffer).  labsort_multi_collectives / labsort_dist_collectives: host wall clock
 * (ms since the rank's call started) at which each rank arrived at / returned from each
 * of them in the last call (-1: did not run); arrive[r * ncoll + k], leave[r * ncoll + k]. */
#define LABSORT_MULTI_COLLECTIVES 3
int labsort_sort_host_multi(void *h_keys, size_t n, int key_type, int ngpus);  /* devices 0..ngpus-1 */
int labsort_sort_host_ranks(void *h_keys, size_t n, int key_type, int nranks, const int *devices, int transport);
int labsort_multi_timing(double *phase_ms, int nphases, size_t *max_sent_bytes);
int labsort_multi_collectives(double *arrive, double *leave, int nranks, int ncoll);
int labsort_multi_last_hip_error(void);
/* keys of each rank's range of the sorted array in the last call (ranks in order) */
int labsort_multi_range_counts(size_t *counts, int nranks);
/* text of the last failure of a multi-GPU call (HIP call, RCCL result, callback) */
const char *labsort_multi_error_detail(void);
/* The exchange plan alone, on host shards (sorted h_shards[r][0..m[r]) per rank;
 * std::upper_bound stands in for the device bound queries): writes the cut points,
 * h_cuts[r*(nranks+1) + j] = first position of the piece rank r sends to rank j.
 * Test hook for the schedule; no GPU involved. */
int labsort_multi_plan(const uint32_t *const *h_shards, const size_t *m, int nranks, int key_type, size_t *h_cuts);

/* One process per GPU (torch.distributed.run / mpirun style): a communicator handle
 * per rank, then one labsort_dist_sort call per rank and sort.
 *   RCCL: rank 0 calls labsort_comm_unique_id, the id (LABSORT_COMM_ID_BYTES) is
 *         broadcast by the caller's own means, every rank calls labsort_comm_init_rccl
 *         with its device current (ncclCommInitRank).
 *   Host callbacks: the collectives are the caller's (labsort_host_coll over host
 *         buffers; device pieces are staged): several ranks may share a GPU (tests).
 * A rank whose own step fails (local sort, samples, bounds, buffers) still reports its
 * status in every collective up to the exchange, so every rank returns an error together
 * (the failed one its own, the others LABSORT_ERR_PEER) instead of waiting for it. */
#define LABSORT_COMM_ID_BYTES 128
/* ranks of one communicator: the receive-side merge takes two halves of at most 8 runs */
#define LABSORT_DIST_MAX_RANKS 16
typedef struct labsort_comm *labsort_comm_t;
typedef struct {
    void *ctx;
    /* h_out[i * bytes .. (i+1) * bytes) = rank i's h_in; return 0 on success */
    int (*allgather)(void *ctx, const void *h_in, void *h_out, size_t bytes);
    /* send_bytes[j] bytes of h_send (pieces back to back in rank order) to rank j,
     * recv_bytes[i] bytes from rank i into h_recv (rank order); own entries are 0 */
    int (*alltoallv)(void *ctx, const void *h_send, const size_t *send_bytes, void *h_recv,
                     const size_t *recv_bytes);
} labsort_host_coll;
int labsort_comm_unique_id(void *id);
/* RCCL communicators are nonblocking (ncclConfig_t blocking = 0): every wait on the peers
 * -- the communicator's creation, each collective, the exchange -- polls
 * ncclCommGetAsyncError and ends at a deadline (LABSORT_COMM_TIMEOUT_S by default).  A
 * rank whose peer never arrives (its transport broke, it left) then returns
 * LABSORT_ERR_PEER and its communicator is aborted (ncclCommAbort: its kernels and proxy
 * stop); later sorts on an aborted communicator return LABSORT_ERR_PEER at once. */
#define LABSORT_COMM_TIMEOUT_S 120.0
int labsort_comm_init_rccl(labsort_comm_t *comm, const void *id, int nranks, int rank);
/* the deadline of every wait on the peers: of `comm`, or (comm NULL) of the in-process
 * ranks' RCCL transport and of the communicators created afterwards */
int labsort_comm_set_timeout(labsort_comm_t comm, double seconds);
int labsort_comm_init_host(labsort_comm_t *comm, int nranks, int rank, const labsort_host_coll *coll);
int labsort_comm_destroy(labsort_comm_t comm);
/* This rank's shard d_keys[0..m) (device, on the comm's device; left untouched) in;
 * out: *d_result = this rank's range of the sorted array (*count keys, global offset
 * *global_offset), in a buffer the communicator owns until its next sort.  Runs on
 * `stream` (ordered after the work already queued there) and returns once the range
 * is complete. */
int labsort_dist_sort(labsort_comm_t comm, const void *d_keys, size_t m, int key_type, void *stream,
                      const void **d_result, size_t *count, size_t *global_offset);
int labsort_dist_timing(labsort_comm_t comm, double *phase_ms, int nphases, size_t *sent_bytes);
/* this rank's arrival / return times at the collectives of its last sort (ncoll entries) */
int labsort_dist_collectives(labsort_comm_t comm, double *arrive, double *leave, int ncoll);
int labsort_dist_last_hip_error(labsort_comm_t comm);
/* TEST HOOK of the multi-GPU schedule (tests only; the product never arms it): rank
 * `rank` of the following labsort_dist_sort / labsort_sort_host_ranks calls fails at
 * `phase` -- "local_sort", "bounds", "recv", "grow" (the receive buffer's growth round) or
 * "exchange" (it leaves without taking part: a broken transport) -- as an out-of-memory
 * or an expired device spin would.  phase NULL disarms; an unknown phase is
 * LABSORT_ERR_ARG.  Process-wide. */
int labsort_test_fault(const char *phase, int rank);

/* ---- key/value (sort_by_key; no lab.cu counterpart, the reference sorts
 * keys only) ----
 * Stable sort of n (key, 4-byte payload) pairs: d_keys_in/d_vals_in -> d_keys_out/
 * d_vals_out (out-of-place or fully in place: keys_in == keys_out and vals_in ==
 * vals_out).  Equal keys keep their input order, so sorting (key, index) pairs gives a
 * stable argsort, from which payloads of any width can be gathered.
 * algo: LABSORT_ALGO_RADIX (8-bit LSD onesweep passes carrying the payload),
 * LABSORT_ALGO_MERGE (LDS tile sort of labsort_pair_tile_keys() pairs + merge-path
 * passes) or LABSORT_ALGO_AUTO (merge up to LABSORT_AUTO_PAIRS_MERGE_MAX_KEYS, radix above).
 * Asynchronous on `stream`, no allocation; d_ws >= labsort_pairs_workspace_bytes(n, algo).
 * key_type LABSORT_KEY_F32: as labsort_sort_device, around the same sort in place on the outputs;
 * an out-of-place call also copies the payloads to d_vals_out first (three more sweeps), and the
 * inputs are not written.  Stable: equal keys, -0.0 and +0.0 apart, NaNs as one value. */
size_t labsort_pair_tile_keys(void);
size_t labsort_pairs_workspace_bytes(size_t n, int algo);
int labsort_sort_pairs_device(const void *d_keys_in, const void *d_vals_in, void *d_keys_out, void *d_vals_out,
                              size_t n, int key_type, int algo, void *d_workspace, size_t workspace_bytes,
                              void *stream);

/* ---- segmented sort: many independent segments of one buffer in one call (batched row
 * sorts, per-row argsort, per-bucket ordering; no lab.cu counterpart, the reference sorts
 * one array) ----
 * Segment i is [d_offsets[i], d_offsets[i+1]); d_offsets holds nseg + 1 words in device
 * memory with d_offsets[0] == 0, d_offsets[nseg] == n and no decrease (empty segments are
 * allowed).  Each segment is sorted on its own in key_type order; the pairs form is stable
 * and carries a 4-byte payload.  Out of place or fully in place (the aliasing rules of
 * labsort_sort_pairs_device).  Asynchronous on `stream`, no allocation, nothing read back:
 * the launch sequence depends on the host arguments only, so a captured call may be
 * replayed on new keys and new offsets in the same buffers.
 * max_segment_keys is the caller's promise about the longest segment (a row sort: the row
 * length).  0 < max_segment_keys <= labsort_segment_tile_keys() (pairs: .._pair_tile_keys())
 * takes the LDS path: every segment is read once, sorted in LDS by the kernel of its length
 * class (one wave / one 256-thread workgroup / one 1024-thread workgroup per segment) and
 * written once.  Anything else (0 = unknown) takes the general path, two stable pair sorts
 * (by key, then by segment id) of the whole array; n <= labsort_max_keys(LABSORT_ALGO_RADIX).
 * n <= 2^31 - 1 and nseg <= 2^31 - 1 on both paths; n == 0 launches nothing and leaves the
 * workspace as it was.
 * The first kernel validates the offsets (ends, order, every length <= max_segment_keys when
 * that is not 0) and sets the workspace's first word on failure; every later kernel of the
 * call then returns without touching the key and payload buffers.
 * labsort_segments_workspace_status synchronises `stream` and returns LABSORT_ERR_ARG for
 * rejected offsets, LABSORT_ERR_DEVICE if an inner pair sort of the general path reported
 * an error, else LABSORT_OK.
 * key_type LABSORT_KEY_F32 on the LDS path: the class kernels take the order image of a key
 * as they load it and undo it as they store it, so the call still reads and writes every key
 * once (NaNs come back as 0x7FFFFFFF).  On the general path the inner pair sorts take the key
 * type (labsort_sort_pairs_device): the keys form writes NaNs as 0x7FFFFFFF, the pairs form
 * gathers the original words. */
/* longest segment the one-pass LDS path sorts (keys only / key+payload) */
size_t labsort_segment_tile_keys(void);
size_t labsort_segment_pair_tile_keys(void);
/* info for tests: the upper length bound of each LDS class, ascending; the last
 * equals the tile size above.  Returns the number of classes. */
int labsort_segment_class_edges(int pairs, size_t *edges, int cap);
size_t labsort_segments_workspace_bytes(size_t n, size_t nseg, size_t max_segment_keys, int pairs);
int labsort_sort_segments_device(const void *d_keys_in, void *d_keys_out, size_t n, const uint32_t *d_offsets,
                                 size_t nseg, size_t max_segment_keys, int key_type, void *d_workspace,
                                 size_t workspace_bytes, void *stream);
int labsort_sort_segments_pairs_device(const void *d_keys_in, const void *d_vals_in, void *d_keys_out,
                                       void *d_vals_out, size_t n, const uint32_t *d_offsets, size_t nseg,
                                       size_t max_segment_keys, int key_type, void *d_workspace,
                                       size_t workspace_bytes, void *stream);
int labsort_segments_workspace_status(const void *d_workspace, void *stream);

/* ---- top-k selection: the k smallest or largest keys of every row, sorted, with their
 * positions (torch.topk on a matrix; no lab.cu counterpart) ----
 * d_keys is a dense rows x cols matrix of 32-bit keys, never written; d_keys_out is rows x k;
 * d_idx_out is rows x k positions within the row, or NULL (keys only).  With
 * u(x) = x ^ flip_of(key_type) ^ (largest ? 0xFFFFFFFF : 0), row r of the output is the first
 * k entries of the stable ascending sort of the row's (u(key), position) pairs, keys written
 * back untransformed: best first, equal keys in order of position, and of the ties of the k-th
 * key those with the lowest positions.  The output, indices included, is a deterministic
 * function of the input (torch.topk leaves the tie order open).
 * key_type LABSORT_KEY_F32: the same with u(x) = ord(x) ^ (largest ? 0xFFFFFFFF : 0), ord as at
 * LABSORT_KEY_F32 above: NaNs are the largest keys, -0.0 is below +0.0, ties (NaNs among
 * themselves included) go by position.  The image is taken where the select's kernels read the
 * input and undone where the k keys are written (no extra pass); NaNs come back as 0x7FFFFFFF.
 * key_type LABSORT_KEY_BF16 / LABSORT_KEY_F16: d_keys is rows x cols and d_keys_out rows x k
 * 16-bit elements (both 2-byte aligned, else LABSORT_ERR_ARG; the overlap checks use these
 * sizes), d_idx_out stays uint32.  u(x) = ord16(x) ^ (largest ? 0xFFFF : 0), ord16 as at
 * LABSORT_KEY_BF16 above; NaNs come back as 0x7FFF.  The kernels that read the input load eight
 * keys per 16 bytes and widen each to (ord16(x) << 16): the select runs two digit levels, not
 * four, and everything behind the input reads keeps its 32-bit layout.  Paths, thresholds,
 * limits and the workspace size are those of the 32-bit key types.
 * 1 <= k <= cols, rows * cols <= 2^31 - 1; rows == 0 or k == 0 launches nothing.
 * LABSORT_ERR_ARG before any launch: NULL d_keys / d_keys_out, a bad key type, k > cols, a
 * missing or short workspace, an output that overlaps the input, d_idx_out == d_keys_out, and
 * rows > 1 with rows * k > labsort_max_keys(LABSORT_ALGO_RADIX) and
 * k > labsort_segment_pair_tile_keys() (the survivors are ordered by the segmented sort's
 * general path).
 * cols <= labsort_segment_pair_tile_keys(): whole rows are sorted in LDS by the segmented
 * sort's class kernels.  Longer rows: an MSD radix select with 8-bit digits (at most one
 * histogram read per digit, no scatter; a row whose surviving bucket fits cols / 8 pairs is
 * narrowed to it), then a stable sort of the k survivors.  k > cols / LABSORT_TOPK_SORT_DIV:
 * whole rows are pair-sorted and the first k copied; the results are identical.
 * Asynchronous on `stream`, no allocation, nothing read back: the launch sequence depends on
 * the host arguments only, so a captured call may be replayed on new keys in the same buffers.
 * The call clears the part of the workspace it relies on (garbage or a reused workspace is fine).
 * labsort_topk_workspace_bytes never shrinks as k grows at fixed rows and cols.
 * labsort_topk_workspace_status synchronises `stream` and returns LABSORT_ERR_DEVICE if an
 * inner sort reported an error (word 0 of the workspace's 256-byte header), else LABSORT_OK. */
#define LABSORT_TOPK_SORT_DIV 4
size_t labsort_topk_workspace_bytes(size_t rows, size_t cols, size_t k);
int labsort_topk_device(const void *d_keys, size_t rows, size_t cols, size_t k, int largest, int key_type,
                        void *d_keys_out, uint32_t *d_idx_out, void *d_workspace, size_t workspace_bytes,
                        void *stream);
int labsort_topk_workspace_status(const void *d_workspace, void *stream);

/* ---- dense row sort: every row of a matrix sorted, stably, with positions
 * (torch.sort(x, dim=-1, descending=..., stable=True); no lab.cu counterpart) ----
 * labsort_topk_device's contract with k = cols and `descending` in place of `largest`: d_keys is a
 * dense rows x cols matrix, never written; d_keys_out is rows x cols; d_idx_out is rows x cols
 * 32-bit positions within the row, or NULL (the keys written are the same either way).  With u
 * as defined at labsort_topk_device, row r of the output is the stable ascending sort of the
 * row's (u(key), position) pairs, keys written back untransformed: equal keys stay in order of
 * position in both directions, NaNs are the largest keys and come back as 0x7FFFFFFF / 0x7FFF,
 * -0.0 is below +0.0.  key_type: all five (U32, I32, F32, BF16, F16); for the 16-bit types d_keys
 * and d_keys_out hold 2-byte elements and need 2-byte alignment only.  This and
 * labsort_sort16_device (below) are the two sorting entries that take the 16-bit types.
 * rows * cols <= 2^31 - 1; rows == 0 or cols == 0 launches nothing (LABSORT_OK before anything
 * else is looked at).  LABSORT_ERR_ARG before any launch: NULL d_keys / d_keys_out, a bad key
 * type, rows > (2^31 - 1) / cols, an odd d_keys / d_keys_out address with a 16-bit type,
 * d_idx_out == d_keys_out, an output that overlaps the input (by the real element sizes), a
 * missing or short workspace.
 * Rows that fit an LDS tile -- cols <= labsort_segment_tile_keys() for the 16-bit types and for
 * 32-bit keys without positions, cols <= labsort_segment_pair_tile_keys() for 32-bit keys with
 * positions -- are sorted by one kernel launch (after the header's clearing): the length class
 * of the segmented sort (labsort_segment_class_edges) is chosen on the host from cols, a row is
 * read once, sorted in LDS and written once, and a key's position is the slot it was loaded into,
 * never read from memory.  A 16-bit key travels as one word, (u(key) << 16) | position, through the
 * keys-only kernels, which sort it on its top two digits only.  Every other shape calls
 * labsort_topk_device with k = cols on the same workspace: the result is the same by contract, the
 * limits and error returns are that call's.
 * Asynchronous on `stream`, no allocation, nothing read back: the launch sequence depends on the
 * host arguments only, so a captured call may be replayed on new keys in the same buffers.
 * labsort_sort_rows_workspace_bytes takes no key type: 256 bytes (the header) for
 * cols <= labsort_segment_pair_tile_keys(), labsort_topk_workspace_bytes(rows, cols, cols) above.
 * labsort_sort_rows_workspace_status synchronises `stream` and returns what
 * labsort_topk_workspace_status returns: LABSORT_OK after an LDS-path call (the header is cleared
 * and nothing sets it), top-k's report after a long-path call.
 * Timing hooks: the LDS path's kernels count under LABSORT_K_SEGSORT. */
size_t labsort_sort_rows_workspace_bytes(size_t rows, size_t cols);
int labsort_sort_rows_device(const void *d_keys, size_t rows, size_t cols, int descending, int key_type,
                             void *d_keys_out, uint32_t *d_idx_out, void *d_workspace, size_t workspace_bytes,
                             void *stream);
int labsort_sort_rows_workspace_status(const void *d_workspace, void *stream);

/* ---- sort of 16-bit rows of any length (bfloat16 / float16 logits of vocabulary length sorted whole,
 * one long score vector argsorted; no lab.cu counterpart) ----
 * labsort_sort_rows_device's contract, restricted to LABSORT_KEY_BF16 / LABSORT_KEY_F16: d_keys is a
 * dense rows x cols matrix of 2-byte elements, never written; row r of the output is the stable
 * ascending sort of the row's (ord16(key) ^ (descending ? 0xFFFF : 0), position) pairs, keys written
 * back untransformed: NaNs are equal, largest and come back as 0x7FFF, -0.0 < +0.0, ties go by
 * position in both directions.  d_idx_out holds rows x cols 32-bit positions within the row, or is
 * NULL (the keys written are the same either way); rows == 1 is the whole-array sort and d_idx_out
 * then its stable argsort.  For every input, keys and positions are bit-identical to what
 * labsort_sort_rows_device writes.
 * rows == 0 or cols == 0 launches nothing (LABSORT_OK before anything else is looked at).
 * LABSORT_ERR_ARG before any launch: any other key type (U32 / I32 / F32 included), and what
 * labsort_sort_rows_device rejects: NULL d_keys / d_keys_out, rows > (2^31 - 1) / cols, an odd
 * d_keys / d_keys_out address (2-byte alignment is enough; rows of odd length start on either 2-byte
 * phase), d_idx_out == d_keys_out, an output that overlaps the input (by the real element sizes), a
 * missing or short workspace.
 * cols <= labsort_segment_tile_keys(): the launch labsort_sort_rows_device makes for the shape (its
 * LDS kernels); the workspace is the 256-byte header.
 * Longer rows: two stable LSD passes with 8-bit digits on u = ord16(key) ^ x16, low byte then high
 * byte.  Rows are independent and cut into chunks of up to labsort_sort16_chunk_keys() consecutive
 * keys (the last may be partial; any cols is fine).  Pass 1 reads d_keys and writes u and, with
 * positions, where each key was loaded from to a temporary in the workspace; pass 2 reads the
 * temporary and writes d_keys_out and d_idx_out.  With d_idx_out == NULL no position is stored or
 * loaded anywhere.  A pass is three launches -- digit counts per (row, chunk) into a table
 * [row][digit][chunk] by plain stores, an exclusive scan of the table along the chunks with the
 * digit totals per row, the scatter of every (row, chunk) -- and no kernel waits on another
 * workgroup: about 24 bytes of memory traffic per key with positions, 12 without.
 * Asynchronous on `stream`, no allocation, nothing read back: the launch sequence depends on the
 * host arguments only, so a captured call may be replayed on new keys in the same buffers.
 * labsort_sort16_workspace_bytes: 256 bytes for cols <= labsort_segment_tile_keys(); above, the
 * header (cleared by the call), the count table (rows x 256 x chunks-per-row words, one table for
 * both passes), the totals, rows * cols * 2 bytes of temporary keys and, with positions,
 * rows * cols * 4 bytes of temporary positions, each region 256-byte aligned.  It never shrinks as
 * rows or cols grow, and a workspace sized with positions serves a call without them.  Garbage or
 * a reused workspace is fine.
 * labsort_sort16_workspace_status synchronises `stream` and reads the header's first word, as the
 * row sort's does; nothing on either path sets it, so it returns LABSORT_OK (it exists so that
 * callers treat every entry alike).
 * Timing hooks: the kernels of both paths count under LABSORT_K_SEGSORT. */
size_t labsort_sort16_chunk_keys(void);   /* keys per (row, chunk) workgroup of the long path; info for tests */
size_t labsort_sort16_workspace_bytes(size_t rows, size_t cols, int with_positions);
int labsort_sort16_device(const void *d_keys, size_t rows, size_t cols, int descending, int key_type,
                          void *d_keys_out, uint32_t *d_idx_out, void *d_workspace, size_t workspace_bytes,
                          void *stream);
int labsort_sort16_workspace_status(const void *d_workspace, void *stream);

/* ---- sort of rows of 8-byte keys of any length (int64 index tensors, packed (src << 32) | dst edge
 * keys, 64-bit hashes, float64 scores; no lab.cu counterpart) ----
 * labsort_sort_rows_device's contract for LABSORT_KEY_U64 / LABSORT_KEY_I64 / LABSORT_KEY_F64 only:
 * d_keys is a dense rows x cols matrix of 8-byte elements, never written; with u(x) = image(x) ^
 * (descending ? ~0 : 0), row r of the output is the stable ascending sort of the row's (u(key),
 * position) pairs, keys written back untransformed (a NaN as 0x7FFFFFFFFFFFFFFF).  d_idx_out holds
 * rows x cols 32-bit positions within the row, or is NULL (the keys written are the same either
 * way); rows == 1 is the whole-array sort and d_idx_out then its stable argsort.
 * rows == 0 or cols == 0 launches nothing (LABSORT_OK before anything else is looked at).
 * LABSORT_ERR_ARG before any launch: any other key type, NULL d_keys / d_keys_out, rows >
 * (2^31 - 1) / cols, a d_keys / d_keys_out address that is not 8-byte aligned, d_idx_out ==
 * d_keys_out, an output that overlaps the input (by the 8-byte and 4-byte extents), a missing or
 * short workspace.
 * Every path runs only the 8-bit digits of u that vary, decided on the device:
 * cols <= C = labsort_sort64_chunk_keys(): one launch after the header is cleared, one workgroup
 * per row: the row is read once, the workgroup ORs u and ~u over its keys, runs the bytes in which
 * both have a bit as stable LSD passes in LDS (a key's position is the slot it was loaded into) and
 * writes the row once.  The plan is per row.  The workspace is the 256-byte header.
 * Longer rows are cut into chunks of up to C consecutive keys (the last may be partial; any cols is
 * fine).  The launch sequence is fixed: the header and the plan are cleared; every chunk ORs u and ~u
 * of its keys into two plan words; one workgroup writes the plan of the call -- the active passes,
 * their number m, and for the j-th of them its source (the input for j == 0, else what the pass
 * before wrote) and its destination (the outputs if m - 1 - j is even, else the temporaries, so the
 * last active pass lands in d_keys_out / d_idx_out whatever m is); then for each byte p = 0 .. 7 a
 * count per (row, chunk) into a table [row][digit][chunk] by plain stores, an exclusive scan of the
 * table along the chunks with the row's digit totals, and the scatter of every (row, chunk), each of
 * which reads the plan and returns at once if pass p is inactive; last a kernel that works only for
 * m == 0 (every key of the call has one image) and writes unord(ord(key)) and the column index.  The
 * first active pass maps keys to images as it loads them and makes positions from where it loaded
 * them, the last one maps back as it stores: about 32 bytes of memory traffic per key and active pass
 * with positions, 24 without.  No kernel waits on another workgroup.  With d_idx_out == NULL no
 * position is stored or loaded anywhere.
 * Asynchronous on `stream`, no allocation, nothing read back: the launch sequence depends on the
 * host arguments only, so a captured call may be replayed on new keys in the same buffers (the plan
 * is decided again on every replay).
 * labsort_sort64_workspace_bytes: 256 bytes for cols <= C; above, the header, the plan, the count
 * table (rows x 256 x chunks-per-row words), the totals, rows * cols * 8 bytes of temporary keys
 * and, with positions, rows * cols * 4 bytes of temporary positions, each region 256-byte aligned.
 * It never shrinks as rows or cols grow, and a workspace sized with positions serves a call without
 * them.  The call clears what it relies on: garbage or a reused workspace is fine.
 * labsort_sort64_workspace_status synchronises `stream` and reads the header's first word; nothing
 * sets it, so it returns LABSORT_OK (it exists so that callers treat every entry alike).
 * labsort_sort64_passes synchronises `stream` and returns the plan of the last call on the
 * workspace as a bitmask, bit p set if the pass on byte p of the image ran; 0 after a short-path
 * call; -LABSORT_ERR_HIP (-LABSORT_ERR_ARG for a NULL workspace) on failure.  For tests and tools,
 * as labsort_radix_path.
 * Timing hooks: the kernels of both paths count under LABSORT_K_SEGSORT. */
size_t labsort_sort64_chunk_keys(void);   /* C: keys per (row, chunk) workgroup; info for tests */
size_t labsort_sort64_workspace_bytes(size_t rows, size_t cols, int with_positions);
int labsort_sort64_device(const void *d_keys, size_t rows, size_t cols, int descending, int key_type,
                          void *d_keys_out, uint32_t *d_idx_out, void *d_workspace, size_t workspace_bytes,
                          void *stream);
int labsort_sort64_workspace_status(const void *d_workspace, void *stream);
int labsort_sort64_passes(const void *d_workspace, void *stream);

/* ---- k-th key selection per row: which key is the k-th of every row, and where it is
 * (torch.kthvalue, the lower median, nearest-rank quantiles, the threshold of top-k masking with a
 * k per request; no lab.cu counterpart) ----
 * d_keys is a dense rows x cols matrix, never written; key_type: all five (U32, I32, F32, BF16, F16),
 * the 16-bit types with 2-byte elements and 2-byte alignment.  d_keys_out holds rows elements of the
 * key type; d_idx_out holds rows 32-bit positions within the row, or is NULL (the keys written are
 * the same either way).  With u as defined at labsort_topk_device (the order image, complemented
 * when `largest`) and k_r the k of row r, row r's output is entry k_r - 1 of the stable ascending
 * sort of the row's (u(key), position) pairs, written back untransformed: key and position are
 * bit-identical to column k_r - 1 of labsort_sort_rows_device(descending = largest).  Among the ties
 * of the k-th key the position is that of the (k_r - count_below)-th occurrence in position order.
 * NaNs are equal, largest and come back as 0x7FFFFFFF / 0x7FFF; -0.0 < +0.0.
 * d_k == NULL: every row uses the host k.  d_k != NULL: rows words in device memory, one k per row,
 * and the host k is ignored.  A d_k[r] outside [1, cols] is clamped into that range by the kernel
 * that reads it, which sets word 0 of the workspace's 256-byte header:
 * labsort_kth_workspace_status (which synchronises `stream`) then returns LABSORT_ERR_ARG, as
 * labsort_segments_workspace_status does for rejected offsets; the other rows' results are valid and
 * nothing is written out of bounds.  Without such a row it returns LABSORT_OK.
 * rows == 0 or cols == 0 launches nothing (LABSORT_OK before anything else is looked at).
 * LABSORT_ERR_ARG before any launch: NULL d_keys / d_keys_out, a bad key type, d_k == NULL with
 * k == 0 or k > cols, rows > (2^31 - 1) / cols, an odd d_keys / d_keys_out address with a 16-bit
 * type, d_idx_out == d_keys_out, an output that overlaps the input, d_k or the other output (by the
 * real element sizes), a missing or short workspace.
 * cols <= labsort_kth_row_keys(): one launch (after the header's clearing), one workgroup per row.
 * The row is loaded once as u and held in registers, every 8-bit digit level (four; two for the
 * 16-bit types) runs on a histogram in LDS, and one ordered scan of the keys equal to the threshold
 * gives the position.  The workspace is the header.
 * Longer rows are cut into chunks of labsort_kth_row_keys() consecutive keys (the last may be
 * partial; any cols and either 2-byte phase is fine).  Per level one kernel counts the level's
 * digit of the keys that match the digits chosen so far, per chunk and per row, and one picks the
 * digit at which the row's running count reaches k.  From the second level on a chunk is read only
 * if it held a key of the digit chosen before; a skipped chunk's counts are zeroed.  With positions
 * the last pick finds, from the chunks' counts, the one chunk that holds the k-th key, and one more
 * kernel reads that chunk in position order; without them the last pick writes the key and no
 * locate kernel runs.  No survivor list, no candidate buffer, no sort, no scatter, and no kernel
 * waits on another workgroup.
 * Asynchronous on `stream`, no allocation, nothing read back: the launch sequence depends on the
 * host arguments only, so a captured call may be replayed on new keys and new d_k values in the
 * same buffers.  The call clears what it relies on in the workspace (garbage or a reused workspace
 * is fine).  labsort_kth_workspace_bytes takes no key type and never shrinks as rows or cols grow:
 * 256 bytes for cols <= labsort_kth_row_keys(); above, the header, rows x 4 x 256 histogram words,
 * the per-row states and rows x chunks x 256 count words (1/16 byte per key), each region 256-byte
 * aligned.
 * Timing hooks: the kernels count under LABSORT_K_TOPK. */
size_t labsort_kth_row_keys(void);      /* longest row the one-launch path takes; info for tests */
size_t labsort_kth_workspace_bytes(size_t rows, size_t cols);
int labsort_kth_device(const void *d_keys, size_t rows, size_t cols, size_t k, const uint32_t *d_k, int largest,
                       int key_type, void *d_keys_out, uint32_t *d_idx_out, void *d_workspace,
                       size_t workspace_bytes, void *stream);
int labsort_kth_workspace_status(const void *d_workspace, void *stream);

/* ---- top-k filtering per row: every row with all but its k best keys replaced by a fill value,
 * and / or the mask of the keys kept (the logits filter of a sampler, with a k per request; no
 * lab.cu counterpart) ----
 * d_keys is a dense rows x cols matrix; key_type: U32, I32, F32, BF16, F16 as for labsort_kth_device
 * (the 64-bit types are LABSORT_ERR_ARG).  With u as defined at labsort_topk_device (the order image,
 * complemented when `largest`) and k_r the k of row r, element i of row r is kept iff (u(key_i), i)
 * is among the first k_r entries of the stable ascending sort of the row's (u, position) pairs: the
 * positions kept are the first k_r columns of labsort_sort_rows_device(descending = largest)'s index
 * output, as a set, so exactly k_r elements of the row are kept.  With (T, P) what labsort_kth_device
 * returns for the row: kept iff u_i < u(T), or u_i == u(T) and i <= P.  NaNs are equal and largest;
 * -0.0 < +0.0.
 * d_keys_out: rows x cols elements of the key type, or NULL.  A kept key is written as the other
 * entries write keys (bit for bit, a NaN as 0x7FFFFFFF / 0x7FFF); every other element becomes
 * fill_bits (16-bit types: its low 16 bits; bits set above them are LABSORT_ERR_ARG).
 * d_keys_out == d_keys filters in place; any other overlap with the input is LABSORT_ERR_ARG.
 * d_mask_out: rows x cols bytes, 1 for kept and 0 otherwise (torch.bool's layout), any alignment, or
 * NULL.  At least one of the two outputs must be given.
 * k, d_k, the clamping of a d_k[r] outside [1, cols], the header word and
 * labsort_topk_mask_workspace_status: exactly as for labsort_kth_device (a clamped row is filtered
 * with the clamped k, the status call returns LABSORT_ERR_ARG, the other rows are valid and nothing is
 * written out of bounds).
 * rows == 0 or cols == 0 launches nothing (LABSORT_OK before anything else is looked at).
 * LABSORT_ERR_ARG before any launch: NULL d_keys, both outputs NULL, a bad key type, d_k == NULL with
 * k == 0 or k > cols, rows > (2^31 - 1) / cols, an odd d_keys / d_keys_out address with a 16-bit type,
 * high fill_bits with a 16-bit type, any overlap (by the real element sizes) between the input, the
 * keys output, the mask output and d_k other than d_keys_out == d_keys, a missing or short workspace.
 * cols <= labsort_kth_row_keys(): one launch (after the header's clearing), one workgroup per row:
 * the select of labsort_kth_device with the row in registers, one ordered scan that ranks the keys
 * equal to the threshold in position order (skipped when all of them are kept), then every thread
 * stores the groups it holds.  Longer rows: labsort_kth_device's launches with positions, their
 * outputs in the workspace, then one streaming kernel over (row, chunk) that tests every element
 * against its row's (T, P).  A group of 16 bytes that lies wholly inside its row is one 16-byte
 * store where the output's address allows it; the heads and tails of rows, which share their
 * 16 bytes with a neighbour row, are stored element by element (no store covers an element of
 * another row, no read-modify-write).  The mask's alignment is tested on its own.  No kernel waits
 * on another workgroup.
 * Asynchronous on `stream`, no allocation, nothing read back; the launch sequence depends on the
 * host arguments only (a captured call replays on new keys and new d_k); the call clears what it
 * relies on in the workspace.  labsort_topk_mask_workspace_bytes never shrinks as rows or cols grow:
 * 256 bytes for cols <= labsort_kth_row_keys(); above, labsort_kth_workspace_bytes' layout and two
 * words per row (the k-th pair's position and key), each region 256-byte aligned.
 * Timing hooks: the kernels count under LABSORT_K_TOPK. */
size_t labsort_topk_mask_workspace_bytes(size_t rows, size_t cols);
int labsort_topk_mask_device(const void *d_keys, size_t rows, size_t cols, size_t k, const uint32_t *d_k,
                             int largest, int key_type, uint32_t fill_bits, void *d_keys_out,
                             uint8_t *d_mask_out, void *d_workspace, size_t workspace_bytes, void *stream);
int labsort_topk_mask_workspace_status(const void *d_workspace, void *stream);

/* ---- top-p (nucleus) filtering per row: every row reduced to the smallest prefix of its most
 * probable elements whose mass reaches p, with a p per request, and / or the mask of the elements
 * kept and their number (the step of a sampler after the softmax; no lab.cu counterpart) ----
 * d_keys is a dense rows x cols matrix of non-negative weights, normally probabilities; key_type:
 * F32, BF16 or F16 (every other type is LABSORT_ERR_ARG), the 16-bit types with 2-byte elements and
 * 2-byte alignment.  All sums are integers, so the result is exact, repeatable and the same in any
 * order of summation:
 * Weight.  An element x weighs w = min(floor(x 2^40), 2^40); 0 if its sign bit is set (-0.0 and -inf
 * too) or if it is a NaN; +inf and everything from 1.0 up weigh 2^40.  The weight is taken from the
 * bit pattern with integer shifts (a 16-bit key as its exact float32 value), on the device and in
 * labsort_top_p_weight (host; 0 for a key type the entry does not take), so neither a denormal mode
 * nor contraction can change it.  cols <= 2^23 keeps a row's total below 2^63; a longer row is
 * LABSORT_ERR_ARG.
 * Target.  W_r is the sum of row r's weights, P_r = clamp(floor(p_r 2^32), 1, 2^32) for the row's
 * float32 p_r (from its bits as well), and t_r = max(1, ceil(P_r W_r / 2^32)), the product in 96 bits.
 * Order.  That of labsort_sort_rows_device(descending = 1): the row's (u, position) pairs ascending,
 * u the complemented order image: NaNs are equal and first, equal keys come in order of position.
 * Kept.  k_r is the smallest n such that the weights of the first n entries of that order sum to at
 * least t_r, and the row keeps exactly those n elements: the outputs are what
 * labsort_topk_mask_device(largest = 1) gives with d_k[r] = k_r, element for element.  Elements of
 * weight zero ahead of the threshold (the NaNs) are kept; those behind the last element with a
 * weight are never kept, not even at p = 1.
 * A row with W_r == 0 is kept whole (k_r = cols) and sets word 0 of the workspace's 256-byte header:
 * labsort_top_p_workspace_status (which synchronises `stream`) then returns LABSORT_ERR_ARG; the other
 * rows' results are valid.  d_p == NULL: every row uses the host p, and a p that is a NaN or outside
 * (0, 1] is LABSORT_ERR_ARG before any launch.  d_p != NULL: rows float32 words in device memory,
 * never written, and the host p is ignored; a d_p[r] outside (0, 1] sets the same header word, with
 * p <= 0 taken as P = 1 and a NaN or p > 1 as P = 2^32.
 * Outputs: any of the three, at least one.  d_keys_out: rows x cols elements of the key type, the
 * kept keys where they were and fill_bits elsewhere; d_keys_out == d_keys filters in place.
 * d_mask_out: rows x cols bytes, 1 for kept.  d_kept_out: rows uint32 words, k_r.  Stores, overlaps,
 * alignment, fill_bits and the NaN spelling of a kept key are labsort_topk_mask_device's.
 * rows == 0 or cols == 0 launches nothing (LABSORT_OK before anything else is looked at).
 * LABSORT_ERR_ARG before any launch: NULL d_keys, all three outputs NULL, a key type other than the
 * three, a bad host p with d_p == NULL, cols > 2^23, rows > (2^31 - 1) / cols, an odd d_keys /
 * d_keys_out address or high fill_bits with a 16-bit type, a d_kept_out or d_p that is not 4-byte
 * aligned, any overlap (by the real element sizes) between the input, the three outputs and d_p
 * other than d_keys_out == d_keys, a missing or short workspace.
 * cols <= labsort_kth_row_keys(): one launch (after the header's clearing), one workgroup per row,
 * the row in registers as u; every digit level sums the weights of the keys that match the digits
 * chosen so far into a histogram of 64-bit masses in LDS and picks the digit d with
 * mass(< d) < t <= mass(<= d), t less mass(< d) going to the next level.  The last prefix is the
 * threshold T, w(T) > 0, and the first ceil(t / w(T)) of its ties in position order are kept, by
 * the top-k filter's ordered scan and stores; the count is one block sum.
 * Longer rows: per level one kernel over (row, chunk) sums each chunk's masses (a chunk without
 * mass in the digit chosen before is skipped) and adds them to the row's, one 64-bit atomic per
 * workgroup and digit, and one kernel per row picks.  The last pick divides each chunk's mass of the
 * last digit by w(T), which is its count of T, finds the chunk that holds the last tie kept and
 * writes the state that labsort_topk_mask_device's last two kernels read: they run as they do there,
 * the streaming pass also counting what it keeps (one atomic per chunk) when d_kept_out is given.
 * No kernel waits on another workgroup.
 * Asynchronous on `stream`, no allocation, nothing read back; the launch sequence depends on the
 * host arguments only (a captured call replays on new keys and a new d_p); the call clears what it
 * relies on in the workspace.  labsort_top_p_workspace_bytes takes no key type and never shrinks as
 * rows or cols grow: 256 bytes for cols <= labsort_kth_row_keys(); above, in this order and each
 * region 256-byte aligned: the header, rows x 4 x 256 histogram masses (8 bytes each), rows x 5
 * 16-byte states of the mass select, rows x 5 16-byte states of labsort_kth_device's layout, rows x
 * chunks x 256 chunk masses (1/8 byte per key), and a position and a key word per row.
 * Timing hooks: the kernels count under LABSORT_K_TOPK. */
uint64_t labsort_top_p_weight(uint32_t word, int key_type);
size_t labsort_top_p_workspace_bytes(size_t rows, size_t cols);
int labsort_top_p_device(const void *d_keys, size_t rows, size_t cols, float p, const float *d_p, int key_type,
                         uint32_t fill_bits, void *d_keys_out, uint8_t *d_mask_out, uint32_t *d_kept_out,
                         void *d_workspace, size_t workspace_bytes, void *stream);
int labsort_top_p_workspace_status(const void *d_workspace, void *stream);

/* ---- categorical sampling per row: positions drawn by exact inverse CDF from caller-supplied random
 * words (the step of a sampler after the filters above: labsort_top_p_device with fill 0 in place,
 * then this call, is a sampler's whole tail; no renormalisation, the call sums the row itself; no
 * lab.cu counterpart) ----
 * d_keys is a dense rows x cols matrix of non-negative weights, never written; key_type: F32, BF16 or
 * F16; addressing, 2-byte alignment of the 16-bit types and cols <= 2^23 as labsort_top_p_device.
 * Weight.  labsort_top_p_weight exactly: w = min(floor(x 2^40), 2^40), 0 for a set sign bit and for a
 * NaN, so a row filtered with fill 0 or a negative fill needs nothing more.  W_r is the row's sum,
 * below 2^63.
 * Random words.  d_u holds rows x ndraw uint32 words in device memory, row-major, never written.  The
 * caller supplies them: the library has no generator.  U is the word itself, uniform in [0, 2^32).
 * Target.  s = floor(U W_r / 2^32), the product (at most 95 bits) from its two 64-bit halves, so
 * 0 <= s < W_r.
 * Draw.  d_idx_out[r * ndraw + d] is the smallest position j whose inclusive prefix w_0 + .. + w_j, in
 * position order, exceeds s.  An element of weight 0 is never drawn.  An element of weight w is drawn
 * for floor or ceil of w 2^32 / W_r values of U.  Every sum is an exact integer, so the result does
 * not depend on how the device adds, repeats bit for bit and can be reproduced on the host.
 * A row with W_r == 0 writes 0xFFFFFFFF to each of its ndraw outputs and sets word 0 of the
 * workspace's 256-byte header: labsort_sample_workspace_status (which synchronises `stream`) then
 * returns LABSORT_ERR_ARG; the other rows' results are valid.
 * rows == 0, cols == 0 or ndraw == 0 launches nothing (LABSORT_OK before anything else is looked at).
 * LABSORT_ERR_ARG before any launch: NULL d_keys, d_u or d_idx_out, a key type other than the three,
 * cols > 2^23, rows > (2^31 - 1) / cols, rows > (2^31 - 1) / ndraw, an odd d_keys address with a
 * 16-bit type, a d_u or d_idx_out that is not 4-byte aligned, any overlap (by the real sizes) between
 * d_keys, d_u and d_idx_out, a missing or short workspace.
 * cols <= labsort_kth_row_keys(): one launch (after the header's clearing), one workgroup per row,
 * the row in registers in 16-byte groups; every thread sums the weights of each group it holds, one
 * ordered 64-bit scan across the workgroup gives every group its range [lo, hi) of the prefix and
 * the row its total, and for each draw the one thread whose group has lo <= s < hi walks its
 * elements and stores the position: no barrier per draw, no histogram, no atomic.
 * Longer rows, three launches: one workgroup per (row, chunk of labsort_kth_row_keys() keys) stores
 * the chunk's mass; one workgroup per row scans the chunk masses (at most 512) into W_r and writes
 * for each draw its chunk and what is left of s inside it; one workgroup per (row, draw) loads that
 * one chunk and searches it as above.  The matrix is read once, plus one chunk per draw.  No kernel
 * waits on another workgroup.  A call with more than 2^21 rows (short rows) or rows x ndraw draws
 * (long rows) sends those workgroups out in several launches of 2^21, so the limits above are the
 * only ones.
 * Asynchronous on `stream`, no allocation, nothing read back; the launch sequence depends on the
 * host arguments only (a captured call replays on new keys and a new d_u); the call clears what it
 * relies on in the workspace.  labsort_sample_workspace_bytes never shrinks as rows, cols or ndraw
 * grow: 256 bytes for cols <= labsort_kth_row_keys(); above, in this order and each region 256-byte
 * aligned: the header, rows x chunks 8-byte chunk masses, rows x ndraw 16-byte draw states (the
 * residual target and the chunk).
 * Timing hooks: the kernels count under LABSORT_K_TOPK. */
size_t labsort_sample_workspace_bytes(size_t rows, size_t cols, size_t ndraw);
int labsort_sample_device(const void *d_keys, size_t rows, size_t cols, const uint32_t *d_u, size_t ndraw, int key_type,
                          uint32_t *d_idx_out, void *d_workspace, size_t workspace_bytes, void *stream);
int labsort_sample_workspace_status(const void *d_workspace, void *stream);

/* ---- unique: the distinct keys of an array with their counts, the position of each one's first
 * occurrence and every element's index into them (torch.unique(return_inverse, return_counts) on
 * index tensors, vocabulary and id compaction, edge deduplication on packed (src << 32) | dst keys,
 * group-by counts; no lab.cu counterpart) ----
 * d_keys holds n elements of the key type, never written.  key_type: U32, I32, F32 (4-byte elements)
 * or U64, I64, F64 (8-byte elements, d_keys and d_unique_out 8-byte aligned); BF16 and F16 are not
 * taken.  Two keys are equal when their order images are equal (labsort_key_order_bits,
 * labsort_key_order_bits64): every NaN is one value, -0.0 and +0.0 are two.
 * flags == 0: d_unique_out[0..m) holds the distinct keys in ascending image order, non-NaN keys
 * untransformed, a NaN as 0x7FFFFFFF / 0x7FFFFFFFFFFFFFFF; d_counts_out[j] the number of occurrences
 * of key j; d_first_out[j] the lowest position i with d_keys[i] equal to it; d_inverse_out[i] = j such
 * that d_unique_out[j] equals d_keys[i]; *d_num_out = m.
 * flags == LABSORT_UNIQUE_CONSECUTIVE: nothing is sorted; entry j describes the j-th run of equal
 * neighbours of d_keys in input order (torch.unique_consecutive under the same equality): the key is
 * from_order_bits(image), the count the run's length, first the run's start, d_inverse_out[i] the run
 * that i lies in, m the number of runs.
 * d_unique_out has room for n elements of the key type, d_counts_out and d_first_out for n words
 * each (the first m are written, nothing behind them is), d_inverse_out for n words, d_num_out for
 * one; d_counts_out, d_first_out and d_inverse_out may each be NULL.  No output may share a byte with
 * the input or with another output, by these extents.
 * n <= labsort_max_keys(LABSORT_ALGO_RADIX) for 4-byte keys, n <= 2^31 - 1 for 8-byte keys.
 * LABSORT_ERR_ARG before any launch: NULL d_keys (n != 0), d_unique_out or d_num_out, a bad key type,
 * an unknown flag bit, a misaligned pointer, an overlap, n past the limit, a missing or short
 * workspace.  n == 0 writes 0 to *d_num_out by one hipMemsetAsync on the stream and nothing else;
 * d_keys may then be NULL and the workspace is not looked at.
 * The default call first sorts: 4-byte keys with d_first_out or d_inverse_out by
 * labsort_sort_pairs_device(LABSORT_ALGO_AUTO) in place on a (key, 0 .. n-1) copy in the workspace,
 * 4-byte keys without them by labsort_sort_device(LABSORT_ALGO_AUTO) into the workspace (no position
 * is stored or loaded anywhere), 8-byte keys by labsort_sort64_device(rows = 1), with or without
 * positions likewise.  Then, over the sorted array (the input in consecutive mode) cut into chunks
 * of C = labsort_unique_chunk_keys() elements: a count of every chunk's run heads (element i is one
 * if i == 0 or its image differs from that of element i - 1, which a chunk's first reads from
 * memory), an exclusive scan of the counts that leaves m in *d_num_out, a kernel that ranks each
 * chunk's heads again and writes keys, first positions, run starts and the inverse, and, with
 * d_counts_out, one that takes the run lengths from the starts (its grid is sized for n; workgroups
 * past m return).  No kernel waits on another workgroup.
 * Asynchronous on `stream`, no allocation, nothing read back: the launch sequence depends on the
 * host arguments only, so a captured call may be replayed on new keys in the same buffers and leaves
 * a new m.  labsort_unique_workspace_bytes: with_positions is non-zero when d_first_out or
 * d_inverse_out will be passed; a workspace sized with positions serves a call without them, and the
 * size never shrinks as n grows.  The call clears or overwrites what it relies on: garbage or a
 * reused workspace is fine.
 * labsort_unique_workspace_status synchronises `stream` and passes on the status of the inner sort of
 * the last call on the workspace (labsort_pairs_workspace_status or labsort_workspace_status for the
 * 4-byte types); LABSORT_OK for the 8-byte types, in consecutive mode and for n == 0.
 * Timing hooks: the kernels of this entry count under LABSORT_K_SEGSORT, the inner sorts' under
 * their own classes. */
#define LABSORT_UNIQUE_CONSECUTIVE 1   /* flags bit 0: do not sort; collapse runs of equal neighbours */
size_t labsort_unique_chunk_keys(void);   /* C: keys per workgroup of the edge passes; info for tests */
size_t labsort_unique_workspace_bytes(size_t n, int key_type, int flags, int with_positions);
int labsort_unique_device(const void *d_keys, size_t n, int key_type, int flags, void *d_unique_out,
                          uint32_t *d_counts_out, uint32_t *d_first_out, uint32_t *d_inverse_out,
                          uint32_t *d_num_out, void *d_workspace, size_t workspace_bytes, void *stream);
int labsort_unique_workspace_status(const void *d_workspace, size_t n, int key_type, int flags, void *stream);

/* ---- searchsorted: the rank of every value in a sorted sequence (torch.searchsorted, torch.bucketize:
 * ids into a compacted vocabulary, isin, CSR row pointers from sorted edge keys, histogram and
 * quantile bins against explicit edges; no lab.cu counterpart) ----
 * d_sorted is seq_rows x cols elements of the key type, each row ascending in image order; d_values
 * is rows x nv elements of the same key type; d_out is rows x nv words.  Neither input is written.
 * seq_rows is rows or 1: with rows, row r of the values is searched in row r of the sequences; with
 * 1, every value is searched in the one sequence (torch.bucketize, and torch.searchsorted with a 1-D
 * sequence).
 * With u the order image (labsort_key_order_bits, labsort_key_order_bits64), d_out[r][j] is the
 * number of elements e of the sequence with u(e) < u(d_values[r][j]) for right == 0, with
 * u(e) <= u(d_values[r][j]) for right != 0.  So every NaN is one value and lies past every number,
 * and -0.0 < +0.0.  torch.searchsorted differs there: it compares floats as the hardware does, so a
 * NaN value ranks by comparisons that are all false and the two zeros are one value.
 * d_sorter is NULL, or seq_rows x cols words: the i-th element of row r in order is
 * d_sorted[r][d_sorter[r][i]], which is what an argsort of the row gives.  A sorter entry >= cols is
 * a caller error; the kernels clamp it to cols - 1, so nothing is read out of bounds.
 * key_type: U32, I32, F32 (4-byte elements, 4-byte aligned), BF16, F16 (2-byte elements, 2-byte
 * aligned), U64, I64, F64 (8-byte elements, 8-byte aligned); d_out and d_sorter are 4-byte aligned.
 * A sequence that is not ascending gives unspecified ranks, yet every rank lies in [0, cols],
 * nothing is read or written out of bounds and nothing hangs: every search makes a number of probes
 * fixed by cols, each clamped into the sequence, whatever the data.
 * Limits: seq_rows * cols <= 2^31 - 1 and rows * nv <= 2^31 - 1.
 * rows == 0 or nv == 0 launches nothing and returns LABSORT_OK before anything else is looked at.
 * cols == 0 writes zeros (one hipMemsetAsync on the stream; d_sorted may then be NULL).
 * LABSORT_ERR_ARG before any launch: a NULL d_sorted (cols != 0), d_values or d_out, a bad key type,
 * seq_rows neither 1 nor rows, a misaligned pointer, d_out sharing a byte with d_sorted, d_sorter,
 * d_values or the workspace by the real extents, a size past the limits, a missing or short workspace
 * (or one not 16-byte aligned) where one is needed.
 * cols <= labsort_searchsorted_row_keys(key_type) (64 KB of images: 16384 4-byte, 8192 8-byte, 32768
 * 2-byte keys): one launch, no workspace (labsort_searchsorted_workspace_bytes is 0, d_workspace may
 * be NULL).  A workgroup stages its sequence's images in LDS once, by 16-byte loads (element by
 * element on an unaligned row or a partial tail, gathered through the sorter), then walks chunks of
 * V = labsort_searchsorted_chunk_values() values: 16-byte loads, eight searches per thread side by
 * side over the LDS array, 16-byte stores.  With one shared sequence the grid is two workgroups per
 * CU, each striding over the chunks; with a sequence per row it is (row, slice of the row's values).
 * Longer sequences: two launches.  The first writes 4096 sample images per sequence, the last
 * element of each of 4096 equal strides (through the sorter), to the workspace: a 256-byte header and
 * seq_rows tables of 4096 images, each 256-byte aligned.  The second stages the table in LDS, finds
 * each value's stride there and finishes inside that stride in global memory by at most
 * floor(log2(stride - 1)) + 1 probes (16 for 2^28 keys), the same predicate on both levels, so that
 * left and right land on the two ends of a run longer than a stride.
 * Asynchronous on `stream`, no allocation, nothing read back: the launch sequence depends on the host
 * arguments only, so a captured call may be replayed on new sequences and new values in the same
 * buffers.  No kernel waits on another workgroup.  The workspace size never shrinks as seq_rows or
 * cols grow, and the call overwrites what it relies on: garbage or a reused workspace is fine.
 * Timing hooks: the kernels count under LABSORT_K_SEGSORT. */
size_t labsort_searchsorted_row_keys(int key_type);    /* longest sequence the LDS path takes; info for tests */
size_t labsort_searchsorted_chunk_values(void);        /* V: values per workgroup step; info for tests */
size_t labsort_searchsorted_workspace_bytes(size_t seq_rows, size_t cols, int key_type);
int labsort_searchsorted_device(const void *d_sorted, size_t seq_rows, size_t cols, const uint32_t *d_sorter,
                                const void *d_values, size_t rows, size_t nv, int right, int key_type,
                                uint32_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- bucket counts: the histogram of values over sorted edges (what torch.bincount of
 * torch.bucketize's ranks gives, without the ranks ever being written; torch.histogram with explicit
 * edges has no GPU form; no lab.cu counterpart) ----
 * d_edges is edge_rows x nedges elements of the key type, each row ascending in image order;
 * d_values is rows x nv elements of the same key type; d_counts_out is rows x (nedges + 1) words.
 * Neither input is written.  edge_rows is rows or 1, as seq_rows is for searchsorted: with rows, row
 * r of the values is counted on row r of the edges; with 1, every row on the one edge row.  The
 * counts are per row of the values either way: a caller who wants one histogram of a whole tensor
 * passes rows = 1.  There is no sorter.
 * d_counts_out[r][b] is the number of j for which labsort_searchsorted_device with the same `right`
 * would have written rank b for d_values[r][j]: bin 0 is "below the first edge", bin nedges "past the
 * last edge"; with right == 0 a value equal to an edge falls in the bin below the edge, with
 * right != 0 in the bin above it.  Every NaN is one value past every number, and -0.0 < +0.0.  Every
 * row of counts sums to nv.
 * key_type: the eight of labsort_searchsorted_device, with its alignment rules (elements aligned to
 * their size, d_counts_out to 4 bytes).
 * Edges that are not ascending give unspecified counts that still sum to nv; nothing is read or
 * written out of bounds and nothing hangs: every search makes a number of probes fixed by nedges.
 * Limits: edge_rows * nedges, rows * nv and rows * (nedges + 1) are each at most 2^31 - 1.
 * rows == 0 launches nothing and returns LABSORT_OK before anything else is looked at.  nv == 0
 * writes zeros (d_values may then be NULL).  nedges == 0 writes nv into each row's single word
 * (d_edges may then be NULL).
 * LABSORT_ERR_ARG before any launch: a NULL d_counts_out, d_values (nv != 0) or d_edges (nedges != 0),
 * a bad key type, edge_rows neither 1 nor rows, a misaligned pointer, d_counts_out sharing a byte with
 * d_edges, d_values or the workspace by the real extents, a size past the limits, a missing or short
 * workspace (or one not 16-byte aligned) where one is needed.
 * nedges <= labsort_bucket_counts_row_edges(key_type) (80 KB of images and counters: 10176 4-byte,
 * 6784 8-byte, 13632 2-byte edges, so that two workgroups fit a CU): one kernel, no workspace
 * (labsort_bucket_counts_workspace_bytes is 0, d_workspace may be NULL).  A workgroup stages its edge
 * row's images in LDS as searchsorted does, keeps nedges + 1 32-bit counters beside them, walks chunks
 * of labsort_searchsorted_chunk_values() values with the same loads and searches and adds each rank
 * into its counter by an LDS atomic, equal neighbouring ranks of a thread first added together in
 * registers.  The grid is (row, slice of the row's values) while the rows are fewer than two
 * workgroups per CU, and the workgroups then add their non-zero counters to the output, zeroed by a
 * kernel of its own (a captured hipMemsetAsync did not replay), with global atomics; with more rows,
 * or rows of one chunk, a workgroup owns its row and stores the counters, zeros included (no zeroing
 * launch then).
 * Longer edge rows: labsort_searchsorted_device's sample kernel (a 256-byte header and edge_rows
 * tables of 4096 images in the workspace), the zeroing of the output, and a kernel that makes
 * searchsorted's two-level search and turns each final rank into a global atomic add, equal
 * neighbouring ranks of a thread combined first.
 * Asynchronous on `stream`, no allocation, nothing read back: the launch sequence depends on the host
 * arguments only, so a captured call may be replayed on new edges and new values in the same
 * buffers.  No kernel waits on another workgroup.  The call zeroes or overwrites the output itself
 * and overwrites what it relies on in the workspace: garbage in either is fine.  The workspace size
 * never shrinks as edge_rows or nedges grow.
 * Timing hooks: the kernels count under LABSORT_K_SEGSORT. */
size_t labsort_bucket_counts_row_edges(int key_type);   /* longest edge row the LDS path takes; info for tests */
size_t labsort_bucket_counts_workspace_bytes(size_t edge_rows, size_t nedges, int key_type);
int labsort_bucket_counts_device(const void *d_edges, size_t edge_rows, size_t nedges,
                                 const void *d_values, size_t rows, size_t nv, int right, int key_type,
                                 uint32_t *d_counts_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- bincount: the same counting without the search (torch.bincount with the length given) ----
 * d_values is rows x nv elements, key_type U32, I32, U64 or I64 only (any other: LABSORT_ERR_ARG);
 * d_counts_out is rows x (nbins + 1) words.  d_counts_out[r][b] for b < nbins is the number of values
 * of row r equal to b; word nbins holds the values outside [0, nbins): negative ones, and those at or
 * past nbins.  Every row of counts sums to nv.  torch.bincount differs: its length follows the
 * largest value, which it reads back, and a negative value is an error there.
 * Limits: rows * nv and rows * (nbins + 1) are each at most 2^31 - 1.  rows == 0 returns LABSORT_OK
 * before anything else is looked at; nv == 0 writes zeros (d_values may then be NULL).
 * LABSORT_ERR_ARG before any launch: a NULL d_counts_out or d_values (nv != 0), a key type not listed,
 * a misaligned pointer, d_counts_out sharing a byte with d_values, a size past the limits.
 * nbins <= labsort_bincount_row_bins() (16384): the counters live in LDS and are flushed as above;
 * past that every run of equal neighbouring values of a thread is one global atomic add on the zeroed
 * output.  No workspace.  The zeroing, graph and timing rules are those of
 * labsort_bucket_counts_device. */
size_t labsort_bincount_row_bins(void);                 /* most bins the LDS path takes; info for tests */
int labsort_bincount_device(const void *d_values, size_t rows, size_t nv, size_t nbins, int key_type,
                            uint32_t *d_counts_out, void *stream);

/* ---- building blocks (exposed for tests and the multi-GPU driver) ---- */
/* Sort every 64-key tile of d_keys in place by 1-bit splits (ballot + mbcnt +
 * ds_permute), stopping early once the tile is sorted: radix_sort_kernel's job. */
int labsort_wave_tile_sort(void *d_keys, size_t n, int key_type, void *stream);
/* Sort every labsort_tile_keys() tile of d_in into d_out (in place allowed). */
int labsort_tile_sort(const void *d_in, void *d_out, size_t n, int key_type, void *stream);
/* One merge pass: runs of `run` keys (power of two, >= labsort_merge_tile_keys()/2)
 * pairwise merged into runs of 2*run.  d_part: >= labsort_merge_parts(n) words. */
size_t labsort_merge_parts(size_t n);
int labsort_merge_pass(const void *d_in, void *d_out, size_t n, size_t run, int key_type, uint32_t *d_part,
                       void *stream);
/* out[0 .. d1-d0) = elements d0 .. d1-1 of merge(A, B) (A before B on ties).
 * d_part: >= labsort_merge_parts(d1-d0) words. */
int labsort_merge(const void *d_a, size_t la, const void *d_b, size_t lb, void *d_out, size_t d0, size_t d1,
                  int key_type, uint32_t *d_part, void *stream);
/* Merge of up to 8 sorted runs lying back to back in d_in: run q =
 * d_in[h_offsets[q] .. h_offsets[q+1]), q < nruns (host array of nruns+1 offsets).
 * Writes the merged keys to d_out[h_offsets[0] .. h_offsets[nruns]) (d_out != d_in);
 * equal keys keep run order (stable): ceil(log2 nruns) levels of pairwise merge-path
 * passes over explicit pairs of runs (k_merge_pass_p, one launch per pair),
 * ping-ponging through the workspace so the last level writes d_out.  Generalises
 * separators_kernel + merge_segments_kernel (lab.cu:209-300) from 2 to K runs; the
 * multi-GPU schedule merges the runs a rank receives with it.
 * d_ws: >= labsort_merge_runs_workspace_bytes(h_offsets[nruns]) (ping-pong keys). */
size_t labsort_merge_runs_workspace_bytes(size_t n);
int labsort_merge_runs(const void *d_in, void *d_out, const size_t *h_offsets, int nruns, int key_type,
                       void *d_workspace, size_t ws_bytes, void *stream);
/* d_hist[p * 2^bits + digit] += count of keys with that digit in pass p
 * (p = 0 .. ceil(32/bits)-1); bits = 8 or 1.  d_hist must be zeroed by the caller. */
int labsort_histogram(const void *d_keys, size_t n, int key_type, int bits, uint32_t *d_hist, void *stream);

/* d_out[i] = number of keys <= d_values[i] in the sorted run d_sorted[0..n) (key order):
 * the cut points of a rank's sorted shard at the common splitters of the multi-GPU
 * exchange (no lab.cu counterpart: the reference is single-GPU). */
int labsort_upper_bound(const void *d_sorted, size_t n, int key_type, const uint32_t *d_values, size_t nv,
                        uint32_t *d_out, void *stream);

/* ---- utilities ---- */
/* Counter-based generator, identical to oracle_fill: keys first..first+n-1. */
int labsort_fill(void *d_out, size_t n, uint64_t seed, int dist, uint64_t param, uint64_t first, void *stream);
/* d_out[0..n) = d_in[0..n) (32-bit words): a streaming copy with 16-B nontemporal loads and
 * stores in 16384-word tiles, one 1024-thread workgroup per CU -- the practical HBM rate of
 * a read-once / write-once pass, which bench.py reports beside each kernel's roofline. */
int labsort_copy(const void *d_in, void *d_out, size_t n, void *stream);
/* *d_count += number of i with key[i] > key[i+1] (0 = sorted). */
int labsort_count_descents(const void *d_keys, size_t n, int key_type, uint32_t *d_count, void *stream);

/* ---- timing hooks (HIP events on the sort's stream) ---- */
int labsort_timing_enable(int on);                /* clears accumulated times */
/* After the stream has been synchronised: total ms and launch count of a
 * kernel class (LABSORT_K_*) recorded since labsort_timing_enable(1). */
int labsort_timing_read(int kernel_class, double *total_ms, long long *launches);

/* ---- the north_star's entry name (the reference never defined it) ---- */
void sort(int *in, int n);

#ifdef __cplusplus
}
#endif
#endif /* LABSORT_H */
