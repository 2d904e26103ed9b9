/*
 * cmf_hip.h -- C ABI of libcmf_hip.so: the MI355X (gfx950) implementation of
 * CMF.jl's convolutive-NMF multiplicative-update (MU) hot path.
 *
 * This is the drop-in boundary.  The reference is pure
 * Julia, so what a maintainer binds is a `ccall` per entry point
 * (INTEGRATION.md shows the Julia side: `struct HIPMultUpdate <: AbstractCFUpdate`).
 * Every entry cites the reference interface it replaces (paths relative to
 * the reference checkout).
 *
 * Conventions
 *   - All host arrays are Julia's own memory layout (column-major, first
 *     index fastest), Float64:
 *         data[n + N*t]          N x T      (Matrix{Float64})
 *         W[k + K*(n + N*l)]     K x N x L  (Array{Float64,3}, "Tensor")
 *         H[k + K*t]             K x T
 *     The device computes in fp32; conversion happens on upload/download.
 *   - Host pointers are borrowed for the duration of the call only.
 *   - Every entry returns 0 on success or a CMF_ERR_* code; the message is
 *     available from cmf_last_error() (thread-local).
 *   - A handle is not re-entrant: one host thread at a time.
 *   - There is no CPU fallback: without a usable HIP device every compute
 *     entry fails with CMF_ERR_HIP.
 *   - Environment.  Everything that selects a code path is an OPTION (cmf_set_option; cmf_option_names lists them).  The library
 *     reads these eleven variables and no others:
 *         CMF_WAIT_TIMEOUT_S     bound of every host-side wait (loss words, helper threads, collectives): seconds, default 300
 *         CMF_WRITEBACK_THREADS  widening helpers of cmf_arm_writeback: default 4, at most 16
 *         CMF_ENQUEUE_THREADS    0: the calling thread enqueues every shard of a one-process group (see cmf_create_multi)
 *         CMF_RCCL_LIB           path of the RCCL to dlopen ("none": behave as if there were no RCCL)
 *         CMF_ROCTX              1: load the roctx marker library and bracket phases and collectives; 0: never; unset: only if the
 *                                process has already mapped it (a profiler)
 *         CMF_TEST_HOOKS         1: honour the test hooks below (and the option "hals_debug"); anything else: they do not exist
 *           CMF_MAX_COLUMNS        columns one handle holds before cmf_create cuts the recording into shards (tests of that path)
 *           CMF_TEST_FORCE_WORKERS 1: an enqueue worker for a ONE-shard RCCL group too
 *           CMF_TEST_FAIL_SHARD    that shard's next all-reduce call fails (tests of the failure path)
 *           CMF_TEST_NO_ARENA      1: every buffer of a handle is an allocation of its own (an overrun cannot hide in a neighbour)
 *           CMF_TEST_N_CU          compute units the launches of every handle cmf_create / cmf_create_shard / cmf_create_multi makes are
 *                                  planned for (the shards of a group included), 1 .. the device's own count; a value outside that
 *                                  range is CMF_ERR_ARG and no handle is made.  Only fewer CUs than exist can be claimed, so every grid
 *                                  still fits the chip (tests of the plans of a partitioned device); cmf_get_counter "plan:n_cu"
 */
#ifndef CMF_HIP_H
#define CMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMF_OK 0
#define CMF_ERR_ARG 1         /* bad argument (null pointer, non-positive size, patience < 1 ...) */
#define CMF_ERR_HIP 2         /* HIP runtime error / no device */
#define CMF_ERR_STATE 3       /* call sequence error (e.g. factors not set) */
#define CMF_ERR_UNSUPPORTED 4 /* shape outside what the kernels implement */
#define CMF_ERR_COMM 5        /* RCCL / collective transport error */

typedef struct cmf_handle_s *cmf_handle;

/* Version of this interface.  3 (round 3): the phase-split entries of version 1 (cmf_w_partial*, cmf_w_apply,
 * cmf_h_update, cmf_loss_partial*, cmf_halo_*, cmf_numden_ptr, cmf_set_data_norm) are gone -- a sharded iteration
 * runs behind the rule entries of a group handle (cmf_create_multi / cmf_comm_init_*); cmf_abi_version,
 * cmf_source_digest, cmf_synchronize, cmf_rccl_version, cmf_get_counter are new.  5 (round 5): cmf_arm_writeback.  6 (round 6):
 * cmf_fingerprint, cmf_option_names, cmf_shard_set_left_data; cmf_set_factors takes one NULL factor; the measurement variables of the environment are gone
 * (CMF_HALS_*, CMF_CONV_*, CMF_SK_*, CMF_GRAM_FW, CMF_PGD_TRANSPOSE, CMF_LOSS_POLL, CMF_SPECULATE_W, CMF_SMALL_K, CMF_HXT_EXACT,
 * CMF_LOOPBACK_*): what tests still select is an option. */
#define CMF_ABI_VERSION 6
int cmf_abi_version(void);

/* Library / build identification: "cmf_hip gfx950 <version> abi=<n> src=<digest>". */
const char *cmf_version(void);
/* Hex SHA-256 prefix (16 characters) of the sources this library was compiled from (csrc/cmf_api.hip, cmf_rules.hip, cmf_groups.hip,
 * cmf_small.hip, cmf_admm.hip, cmf_anls.hip, cmf_sep.hip, cmf_xortho.hip, cmf_events.hip, cmf_signif.hip, cmf_recentre.hip, cmf_options.hip, cmf_internal.h, cmf_kernels.h, cmf_conv_modes.h, cmf_small_k.h, cmf_workers.h, cmf_writeback.h, cmf_rng.h, cmf_fp64.h, cmf_admm.h, cmf_anls.h, cmf_nnls_large.h, cmf_sep.h, cmf_xortho.h, cmf_events.h, cmf_mu_install.h, cmf_signif.h, cmf_recentre.h, cmf_options.h, include/cmf_hip.h, in that order, each preceded by its base name and a newline).
 * A loader that has the tree at hand recomputes it and refuses (or rebuilds) a stale binary -- cmf.jl_amd/_lib.py does;
 * "unknown" when the library was built without the build script. */
const char *cmf_source_digest(void);
/* Message of the last failing call on this thread ("" if none). */
const char *cmf_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unusable). */
int cmf_device_count(void);

/* ---- rule construction -------------------------------------------------
 * Replaces the MultUpdate constructor `MultUpdate(data, W, H)`
 * (src/algs/mult.jl:11-20, called at src/model.jl:79): uploads `data`
 * (N x T), allocates the rule's scratch (est, numW, denomW, numH, denomH)
 * on `device`, and computes data_norm = norm(data).
 * cmf_create is the single-GPU form of cmf_create_shard.  A recording with more columns than one handle's 32-bit buffer
 * offsets reach (8.3 M at K <= 64) is cut along T into several shards on the SAME device automatically (the handle then fronts
 * a loopback group, see cmf_create_multi): the MU and PGD rules run on it unchanged, HALS -- whose H sweep is one chain along
 * T -- reports that it cannot. */
int cmf_create(cmf_handle *h, int device, int64_t N, int64_t T, int64_t K, int64_t L,
               const double *data);

/* T-sharded form: this handle owns global columns
 * [t_offset, t_offset + T_local) of a T_global-column problem.
 * `data_local` holds columns [t_offset, t_offset + T_local + halo_r) where
 * halo_r = min(L-1, T_global - t_offset - T_local) (the static right halo of
 * `data` that tensor_transconv needs).  The shard joins its group with cmf_comm_init_rccl /
 * cmf_comm_init_callbacks (below), which also all-reduces data_norm. */
int cmf_create_shard(cmf_handle *h, int device, int64_t N, int64_t T_local, int64_t K, int64_t L,
                     const double *data_local, int64_t t_offset, int64_t T_global);
/* The L-1 columns of data in FRONT of a shard (N x (L-1), columns [t_offset - (L-1), t_offset); the shard with t_offset = 0 has none and
 * need not call this).  With them resident on every shard -- call it between cmf_create_shard and cmf_comm_init_* -- the group carries
 * the halo of H in the tail of its W-phase all-reduce (ONE collective per iteration; see the group section below) instead of in an
 * all-gather of its own behind every H update.  cmf_create_multi does this itself.  No reference counterpart. */
int cmf_shard_set_left_data(cmf_handle h, const double *cols);

/* ---- T-sharded groups: the same rule on several GPUs of one node -----------------
 * The T axis of data / est / H is cut into contiguous column blocks (shard r owns columns
 * [r*ceil(T/R), min(T, (r+1)*ceil(T/R)))), W is replicated.  Per MU iteration the shards meet ONCE: one RCCL
 * all-reduce of the [numW | denomW] partial sums (2*L*Kpad*Npad floats) + a tail that carries every shard's loss
 * partial of the previous iteration and -- since round 6 -- every shard's outer columns of the new H (its last 2(L-1) and
 * first L-1: 7.3 KB per rank at config 2), so that no exchange stands between the H update and the loss conv: every shard
 * with a left neighbour updates the L-1 columns in front of its own itself (0.6 - 2 % redundant work on a T/8 shard).
 * That form (option "halo_in_allreduce", default on) needs K a multiple of 32, 1 <= L-1 <= 64, shards of at least 2(L-1)
 * columns and the default formulation; otherwise, and for the Gram form and the PGD rule, the (L-1)-column halos travel in
 * an all-gather of their own behind every H update (2 x 2.4 KB per shard), as they did until round 5.
 * cmf_get_counter "allreduce_calls" / "allgather_calls" count the collectives a handle has issued, "halo_in_allreduce" says
 * which form is in force.
 * On a group handle cmf_set_factors / cmf_get_factors / cmf_update_motifs / cmf_update_feature_maps /
 * cmf_compute_loss / cmf_iterate / cmf_fit run the whole sharded iteration including the collectives, so the
 * reference's `fit` loop (src/algs/alternating.jl:44-67: one update_motifs! and one update_feature_maps! per
 * iteration) drives all GPUs with the same two calls.
 *
 * cmf_create_multi: ONE process drives `ndev` shards (the rule constructor `MultUpdate(data, W, H)`,
 * src/algs/mult.jl:11-20, for a Julia task).  devices[r] is the HIP device of shard r; `data` is the whole N x T
 * matrix, H crosses the ABI as the whole K x T matrix.  transport: CMF_COMM_AUTO = RCCL (ncclCommInitAll, one
 * stream per device, collectives inside ncclGroupStart/End) when the devices are distinct, loopback when they
 * are all the same device (the shards then share that device and the collectives are plain kernels: middle-rank
 * shards on a one-GPU box); CMF_COMM_RCCL forces RCCL (a 1-device group then still sends its buffers through
 * RCCL); CMF_COMM_LOOPBACK forces loopback (devices must all be equal). */
#define CMF_COMM_AUTO 0
#define CMF_COMM_RCCL 1
#define CMF_COMM_LOOPBACK 2
#define CMF_COMM_LOOPBACK_STREAMS 3 /* loopback with a stream per shard: the collectives keep RCCL's stream semantics (start when
                                       every shard's stream has arrived, every shard's stream continues when done) through
                                       events, so a missing dependency between shards cannot hide behind a shared stream */
#define CMF_COMM_PEER 4 /* direct peer access instead of RCCL (opt-in; one-process groups only): hipDeviceEnablePeerAccess between
                           all devices, the all-reduce is ONE kernel per device that sums its 1/R slice from the R buffers (reads
                           over xGMI) and stores the result into all of them (writes over xGMI) -- 1/R of the payload per link and
                           direction where a ring moves (R-1)/R of it twice -- between two event fences of all streams; visibility by
                           kernel boundaries only.  Sums in rank order: bitwise the loopback transport's results.  `devices` may also
                           list ONE device ndev times (rehearsal of the protocol on a one-GPU box).  RCCL stays the default: this
                           transport has never run across distinct devices. */
/* Who enqueues: groups whose shards have a stream each (RCCL, peer, loopback-streams) start one ENQUEUE WORKER thread per
 * shard; the calling thread only posts a shard's share of a phase to its worker, which issues the kernels and that shard's
 * collective calls (RCCL's one-thread-per-device mode: no ncclGroupStart/End).  cmf_set_option(h, "enqueue_threads", 0) or
 * CMF_ENQUEUE_THREADS=0 in the environment: the calling thread enqueues all shards, collectives in grouped calls.  Either
 * way a handle is used by one host thread at a time, every call returns with its work handed to the streams, and results
 * are bitwise the same. */
int cmf_create_multi(cmf_handle *h, int ndev, const int *devices, int transport,
                     int64_t N, int64_t T, int64_t K, int64_t L, const double *data);

/* One process per shard (torchrun-style launchers): create the shard with cmf_create_shard, then attach the
 * communicator.  cmf_comm_unique_id writes the 128-byte ncclUniqueId (rank 0 calls it and hands the bytes to the
 * other ranks by any out-of-band means); cmf_comm_init_rccl is ncclCommInitRank on the handle's device.  Both
 * all-reduce the data norm; H crosses the ABI as the LOCAL K x T_local block. */
int cmf_comm_unique_id(void *id128);
int cmf_comm_init_rccl(cmf_handle h, int nranks, int rank, const void *id128);
/* The overlap form (option "allreduce_overlap") runs its bulk all-reduce on a second stream while collectives of the main
 * stream are issued: that stream gets a communicator of its OWN, so that no two collectives in flight ever share one.
 * One process per shard: every rank calls this once with a SECOND id (rank 0's cmf_comm_unique_id, handed over like the
 * first) before switching the option on -- without it the option is refused (CMF_ERR_STATE).  cmf_create_multi groups
 * create their second set of communicators themselves (a second ncclCommInitAll) when the option is switched on.
 * No reference counterpart: the reference has no distributed code. */
int cmf_comm_init_overlap(cmf_handle h, const void *id128);
/* Host-collective transport (MPI / gloo style, used by the multi-process tests on one GPU): the library stages
 * each buffer through pinned host memory and calls back.  allreduce sums `count` floats in place over all ranks;
 * allgather fills recv (nranks * count floats, rank order) from every rank's `count`-float send block.  A non-zero
 * return aborts the entry with CMF_ERR_COMM. */
typedef int (*cmf_allreduce_fn)(void *user, float *host_buf, int64_t count);
typedef int (*cmf_allgather_fn)(void *user, const float *host_send, float *host_recv, int64_t count);
int cmf_comm_init_callbacks(cmf_handle h, int nranks, int rank, cmf_allreduce_fn allreduce, cmf_allgather_fn allgather, void *user);
/* "transport=rccl version=2.x.y lib=/path/librccl.so nranks=8 local=1 ranks=3" (truncated to len). */
int cmf_comm_info(cmf_handle h, char *buf, int64_t len);
/* Column block [t0, t1) of shard `rank` of a group handle (of the handle itself when it is not a group). */
int cmf_shard_bounds(cmf_handle h, int rank, int64_t *t0, int64_t *t1);

int cmf_destroy(cmf_handle h);

/* Block until everything this handle has enqueued -- on every stream of every local shard of a group -- has finished. */
int cmf_synchronize(cmf_handle h);
/* RCCL as this process would bind it (dlopen at first use, a copy the process has already mapped wins): its version
 * code (e.g. 22703) and, when path != NULL, the file it was loaded from.  CMF_ERR_COMM when no RCCL can be loaded. */
int cmf_rccl_version(int *version, char *path, int64_t path_len);
/* Event counters of a handle.  "hals_pipeline_reruns": H sweeps whose persistent pipeline ran out of a bounded wait and
 * were redone from the snapshot on the stage pipeline (cmf_hals_update_feature_maps).  "liveness_checks" (process-wide): stream queries the
 * waits for a loss have made -- 0 in a healthy run whose losses arrive within 50 ms (a query per iteration cost the device a marker
 * packet behind every loss conv until round 6).  "small_k_fused_h_updates": H updates of
 * the MU rule that ran inside the few-component contraction launch (option "small_k_fuse").  Group handles: "enqueue_ns" /
 * "enqueue_iters" = nanoseconds the calling thread spent enqueueing (or posting to the enqueue workers) the pipelined
 * iterations of cmf_iterate, and how many iterations that covers; "worker_ns" = time the busiest enqueue worker spent
 * inside its jobs (0 without workers).  "launches:<path>" (a group: over its shards): launches of one kernel path, counted on the
 * host at the launch site (observability for tests; no device work).  Instances and forms count separately, so one launch adds to
 * several names:  conv_kernel (K % 32 != 0), conv2_kernel, conv3_kernel:whole, conv3_kernel:whole+4, conv3_kernel:whole+16,
 * conv3_kernel:pieces4, conv3_kernel:pieces16 (whole 64 x 64 tiles only / with the grid's tail cut into quarter or sixteenth
 * pieces / pieces only);  conv_small_kernel<NKP> (NKP 1, 2, 3, 4, 6, 8), conv_small_kernel:quarter, conv_small_kernel:pre;
 * hxt_kernel<LP> (LP 1, 2, 3, 4, 5, 6, 8), hxt_kernel:nsrc1, hxt_kernel:nsrc2, hxt_kernel:tail, hxt_kernel:no_tail (rows past
 * the last whole ring rotation left to the slab sum, or none);  transconv_kernel<LT> (LT 4, 8, ..., 32),
 * transconv_kernel:front_block, transconv_kernel:xcd (the plan's XCD placement);  hxt_small_kernel<MBW> (1 .. 10),
 * hxt_small_kernel<MBW,RV> (1 .. 3: with VALU rows), g_gemm_fold_small_kernel<MBW> (1 .. 6), g_gemm_fold_small_kernel<MBW,RV>
 * (1 .. 3), g_gemm_fold_small_kernel:split (the reduction over n in more than one piece), g_gemm_fold_small_kernel:fused_h;
 * gram_w_kernel, gram_lag_corr, gram_w_taps, gram_h_mfma_kernel, gram_h_kernel;  slab_sum_kernel, slab_sum_kernel:carry,
 * slab_sum_small_kernel, slab_sum_small_kernel:carry (with a deferred loss reduction riding on it);  halo_pack2_kernel,
 * halo_unpack2_kernel, halo_pack3_kernel, halo_unpack3_kernel.  An unknown path is CMF_ERR_ARG.
 * "plan:n_cu": the compute-unit count the handle's launches are planned for -- the device's multiProcessorCount, or the test hook
 * CMF_TEST_N_CU (a group: the value of its shards). */
int cmf_get_counter(cmf_handle h, const char *name, int64_t *value);

/* Run all work of this handle on an existing HIP stream (hipStream_t passed
 * as void*), e.g. torch's current stream.  NULL is the HIP null (legacy
 * default) stream -- which is what torch's default "current stream" is.
 * A new handle runs on a private non-blocking stream until this is called.  A change of stream first waits for what the handle
 * has enqueued on the stream it leaves (a rule call may return with the next call's contraction in flight: option "speculate").
 * Group handles refuse it (CMF_ERR_STATE): they run on their own per-shard streams, and that includes the handle
 * cmf_create returns for a recording longer than one handle addresses (T > 8.3 M columns at K <= 64, see cmf_create) --
 * a caller that orders work through torch's current stream must cmf_synchronize such a handle instead. */
int cmf_set_stream(cmf_handle h, void *hip_stream);

/* Options (name, value):
 *   "reuse_est" (default 1): the est = tensor_conv(W, H) that closes update_feature_maps!
 *       (mult.jl:55) is kept, and the next update_motifs! (mult.jl:28), which would recompute the
 *       same est from the same W and H, reuses it (6 instead of 7 contractions per iteration,
 *       identical results).  0 = recompute it like the reference does.
 *   "speculate" (default 1): when the caller alternates update_motifs! / update_feature_maps! (alternating.jl:51-54), the latter
 *       enqueues the contraction the next update_motifs! starts with (numerator and denominator of mult.jl:31-34 need H, data and
 *       est only; l1W, l2W enter afterwards) behind its loss conv, so that the device works while the loss travels to the host and
 *       the caller's loop comes round; update_motifs! then only applies the update.  Identical results; anything that changes W, H,
 *       est or an option in between discards the work.  Single-GPU handles, with "reuse_est": the MU rule, and the HALS rule
 *       (hals.jl:13-38: the contraction of the residual with H_unfold and the lag correlations of H).  A caller that stops
 *       after an update_feature_maps! pays one contraction nobody reads (cmf_get_counter "speculated_contractions" counts the hits).
 *   "gram" (default 0): 1 = form denomW and denomH through Gram matrices (denomW = (H_unfold H_unfold') W,
 *       denomH = lag-Gram taps of W applied to H) instead of through est: exact rewritings of mult.jl:33,48 that
 *       execute 2.3 instead of 6 contractions plus the loss conv; results differ at rounding level only.
 *       2 = additionally take the loss from <H, denomH> - 2<H, numH> + ||data||^2 (no conv at all; the fp32
 *       cancellation limits its relative accuracy to about 1e-6 / loss^2; measured <= 5e-7 on the test shapes).  gram = 1 is
 *       also available on group handles: the all-reduce then carries [numW | HH | tail] (HH = H_unfold H_unfold', every
 *       shard's additive share) instead of [numW | denomW | tail]; it needs T >= 4 L.  gram = 2: unsharded handles only.
 *   "conv_kernel" (default 0 = chosen per launch; 2 = 128 x 128 workgroup tiles for the launches that only store or only
 *       sum the loss -- the epilogues that read data and store always take the one-wave kernel; 3 = one-wave 64 x 64 tiles) and
 *   "conv_split" (default 1: the tiles at the end of the one-wave kernel's grid -- a thin last round, and from four
 *       rounds on three more tiles per CU -- are cut into 32 x 32 quarter or 16 x 16 sixteenth tiles; 4 = quarter tiles
 *       only; 0 = whole tiles only): kernel selection of tensor_conv, for measurements.
 *   "small_k" (default 1 where it applies: K <= 16 and L <= 64): the few-component kernels (csrc/cmf_small_k.h) -- the three
 *       contractions of mult.jl:28-34,44-55 with the FLATTENED (lag, component) index on the MFMA axes instead of K padded to 32:
 *       the shapes the reference publishes on (README.md K = 5; figures/fast_bcd/synthetic_comparison.jl:58-64) run 2-3 times
 *       faster.  tensor_transconv keeps the general kernel when T is too short to fill the chip with its GEMM form; 2 = the
 *       few-component form whatever T is; 0 = the general kernels for every K.  Same arithmetic, another summation order.
 *   "small_k_fuse" (default 1): with the few-component kernels the element-wise update of H (mult.jl:51-52) runs inside the
 *       launch of the contraction before it -- the workgroup that completes a 128-column block's partial sums updates the
 *       block -- instead of in a launch of its own, where that launch is several rounds of workgroups long; bit for bit the
 *       same H (0 = the separate launch always; 2 = the fused form also on short launches, where it is slower; tests compare).
 *   "hals_prepare": allocate the HALS rule's scratch and check its shape limits now (see the HALS entries).
 *   "hals_persist" (default 1): how the H sweep of the HALS rule runs.  1 = as ONE persistent launch where its grid fits the chip
 *       (K sweepers + 4 (K-1) pullers, one workgroup per CU), 0 = one launch per pipeline stage, n > 1 = the persistent launch with at
 *       most n puller workgroups per row.  "hals_seg" (default 384; rounded up to a multiple of 64, at least 256) and "hals_lag"
 *       (default 2; 3 = the unshifted schedule) shape the stage pipeline; "hals_general" (default 0; bit 0 / bit 1) forces the general
 *       W / H sweeps at shapes the on-chip sweeps cover.  All four give the reference's visiting order and agree to rounding (the
 *       tests compare them); they exist for tests and measurements.  "hals_debug" (needs CMF_TEST_HOOKS=1; results are WRONG by
 *       design): 3 = the pullers of the persistent launch leave at once, so that every bounded wait runs out (the test of that
 *       path); 1 / 2 = no gating / pullers skip their work (timing).
 *   "hals_chase" (default -1 = a share estimated from the shape, 64 at config 5; 0 = off; 1..100 = that share): per cent of the tile rows of the residual conv behind the H sweep (hals.jl:41: the residual
 *       and the loss) that CHASE the persistent row pipeline instead of waiting for it: the pipeline (K + 4 (K-1) workgroups, VALU
 *       only) runs on a stream masked to the CUs it needs, those tile rows on a stream masked to the others, each tile waiting for
 *       the last row's progress flag; the rest of the conv follows on the whole chip (the pipeline then runs with three pullers per row instead of four: +1 % of its
 *       span for 32 more CUs on the conv's side).  The same arithmetic per tile (the two launches cut
 *       other tiles of their grids' tails into pieces: sums agree to rounding; run to run the results are bit for bit the same).
 *       K a multiple of 32, T >= 4096.
 *   "hals_gram" (default 2): where the HALS sweeps' projections come from.  2 = P of the H phase as denomH - numH of the MU
 *       quantities (one conv launch less; H within the residual form's accuracy), G of the W phase contracted from the
 *       stored residual; 0 = both from the residual; 1 = both as differences (no residual at all, but about 20x the
 *       rounding error in W).  ACCURACY: 0 and 2 meet the north star's 1e-4 (fp32 against the fp64 reference arithmetic)
 *       on W, H and loss_hist; hals_gram = 1 does NOT -- it is held to 3e-4 in the tests (measured: W 4-8e-5, H up to
 *       1.4e-4) and exists for measurements only.
 *   "profile" (n): bracket every n-th contraction launch with HIP events (cmf_kernel_times); 0 stops.
 *   "profile_mask" (bits): the kernel classes "profile" times -- bit i = the i-th name of cmf_kernel_times ("conv", "conv_t",
 *       "conv_loss", "conv_loss_store", "hxt", "transconv", ...); 0 (default) = all.  (An event pair idles the device a few
 *       microseconds: bench.py times only the dominant kernel inside its timed steps.)
 *   "halo_in_allreduce" (group handles, default 1): 0 = the halo of H in an all-gather of its own behind every H update (the form of
 *       rounds 1-5) even where the all-reduce could carry it (see the group section above).
 *   "allreduce_overlap" (group handles, default 0): 1 = numW (which needs H only) is contracted and all-reduced on a
 *       second stream right after the H update, underneath the loss conv and the denominator contraction, so only
 *       the denomW half of the all-reduce stays exposed; costs a second C2 launch per iteration. */
int cmf_set_option(cmf_handle h, const char *name, int value);
/* The names cmf_set_option accepts, comma-separated (truncation is an error: CMF_ERR_ARG; 512 bytes are plenty). */
int cmf_option_names(char *buf, int64_t len);

/* sum(data.^2) (fp64) over the columns this handle owns -- over all shards on a group handle
 * (data_norm: src/algs/mult.jl:13). */
int cmf_get_data_sumsq(cmf_handle h, double *sumsq);

/* ---- factors -------------------------------------------------------------
 * W (K x N x L) and H (K x T_local) in / out.  `fit` deep-copies the
 * initial factors and the rule mutates them in place
 * (src/algs/alternating.jl:33-34, src/algs/mult.jl:37-38,51-52): here the
 * working copies live on the device between calls.  cmf_set_factors: one of W, H may be NULL once both have been set -- that
 * factor keeps its resident value (a caller that edited only H between two rule calls uploads only H).  cmf_get_factors: either
 * may be NULL (not downloaded). */
int cmf_set_factors(cmf_handle h, const double *W, const double *H);
int cmf_get_factors(cmf_handle h, double *W, double *H);
/* The reference's rules READ the W and H they are handed (src/algs/mult.jl:23,42; hals.jl:31,37; pgd.jl:158,180); here the working
 * copies are device-resident, so a binding that wants the reference's semantics must notice when the caller hands it other arrays,
 * or arrays it has edited, and upload them first.  cmf_fingerprint is the cheap test the bindings use (CMFHip.jl `sync_args!`,
 * host.py `_sync_args`): a 64-bit fingerprint of a Float64 array of n elements over every line_stride-th 64-byte line (8 elements),
 * the last line and n itself (line_stride 1 = every element; the bindings' default 64 reads one line per 4 KB: 360 KB of the 23 MB
 * of factors at config 2).  Host arithmetic only (no handle, no device); equal arrays give equal fingerprints on every machine. */
int cmf_fingerprint(const double *a, int64_t n, int64_t line_stride, uint64_t *fingerprint);

/* In-place semantics for a caller that drives the rule call by call (the reference's own `fit`, src/algs/alternating.jl:51-54,
 * hands the SAME W and H arrays to every call and the rules mutate them: src/algs/mult.jl:37-38,51-52; hals.jl:110,153;
 * pgd.jl:293).  cmf_arm_writeback(h, W, H), called after update_motifs! and immediately before update_feature_maps! of any
 * rule (cmf_update_feature_maps, cmf_hals_update_feature_maps, cmf_pgd_update_feature_maps), makes THAT call also write the
 * new factors into W (K x N x L) and H (K x T), bit for bit what cmf_get_factors returns, before it returns -- without the
 * 23 MB synchronous fp64 download at config 2: W travels (fp32, pinned memory, a copy stream) underneath the H phase's first
 * contraction, H underneath the loss conv, and helper threads widen to Float64 while the caller waits for the loss scalar.
 * Either pointer may be NULL (that factor is not written); both NULL disarms.  EXCEPTION to "host pointers are borrowed for
 * the duration of the call only": W and H are borrowed from this call until the next *_update_feature_maps call on the handle
 * returns, and are written only inside that call.  One arm serves one call; cmf_iterate and cmf_fit (which run H phases of their own, not the
 * caller's rule calls) drop an arm that is still standing at their entry and write nothing.  If a helper thread ever fails to return within
 * CMF_WAIT_TIMEOUT_S (a hung device), the call fails and the handle refuses further arms (CMF_ERR_STATE); cmf_get_factors still works.
 * On a group handle (MU rule in either formulation, PGD rule)
 * every shard copies its own column block of H on its own device the same way (shard 0 also W) and the handle's helpers widen
 * block after block.
 * CMF_WRITEBACK_THREADS (environment, default 4): the widening helpers.
 * cmf_get_counter: "writeback_calls", "writeback_overlapped" (calls served by the copy stream). */
int cmf_arm_writeback(cmf_handle h, double *W, double *H);

/* ---- the update rule -------------------------------------------------------
 * update_motifs!(rule::MultUpdate, data, W, H; l1W=0, l2W=0)
 *   src/algs/mult.jl:23-39  (called at src/algs/alternating.jl:52). */
int cmf_update_motifs(cmf_handle h, double l1W, double l2W);
/* update_feature_maps!(rule::MultUpdate, data, W, H; l1H=0, l2H=0) -> loss
 *   src/algs/mult.jl:42-58  (called at src/algs/alternating.jl:54).
 * Synchronises: *loss is valid on return. */
int cmf_update_feature_maps(cmf_handle h, double l1H, double l2H, double *loss);
/* compute_loss(data, W, H) = norm(tensor_conv(W,H) - data) / norm(data)
 *   src/common.jl:54-59 (loss_hist[1], src/algs/alternating.jl:37). */
int cmf_compute_loss(cmf_handle h, double *loss);

/* The whole loop of fit(::AlternatingOptimizer, ...) with W, H device-resident:
 *   src/algs/alternating.jl:16-71.  loss_hist/time_hist must hold max_itr+1
 * doubles; *n_hist receives the number of entries written (iterations + 1);
 * *converged_early is 1 when the loop stopped on `converged` (:63-66; the
 * host wrapper prints "Converged early." like the reference).
 * Valid on single-GPU and group handles (on a group with a finite max_time every rank follows rank 0's clock).
 * time_hist: with a stop test armed (check_convergence != 0 or a finite max_time) entry i is the reference's cumulative
 * wall-clock time around the two rule calls of iteration i (alternating.jl:49,57-58).  When neither test can fire the loop runs
 * as ONE pipelined cmf_iterate batch (the host never stalls the device between iterations) and entry i is the DEVICE time,
 * from the start of the batch, at which iteration i was complete -- a HIP timing event recorded behind that iteration's loss
 * conv (shard 0's stream on a group) -- i.e. the same quantity without the host in it.  (Batches of more than 8192 iterations
 * keep host times: the moment each loss reached the host, half an iteration late.) */
int cmf_fit(cmf_handle h, int64_t max_itr, double max_time,
            int check_convergence, int64_t patience, double tol, int eval_mode,
            double l1W, double l2W, double l1H, double l2H,
            double *loss_hist, double *time_hist, int64_t *n_hist, int *converged_early);

/* n_iter MU iterations back to back: exactly `update_motifs!; update_feature_maps!` (alternating.jl:51-54; eval_mode
 * skips the motif update like :51) n_iter times, losses[i] = the loss update_feature_maps! returned in iteration i.
 * The host does not stall the device between iterations: the loss of iteration i is read one iteration late from
 * pinned memory (on a group handle it travels in the tail of iteration i+1's all-reduce, so an iteration costs one
 * all-reduce -- which also carries the halos of H, see the group section -- and one host wait).  stamps (may be NULL):
 * seconds since entry at which each loss
 * became known to the host.  cmf_fit uses this loop when check_convergence is 0 and max_time is infinite. */
int cmf_iterate(cmf_handle h, int64_t n_iter, int eval_mode, double l1W, double l2W, double l1H, double l2H,
                double *losses, double *stamps);

/* ---- HALS rule (BASELINE config 5) ----------------------------------------------
 * update_motifs!(rule::HALSUpdate, data, W, H; l1W=0, l2W=0)            src/algs/hals.jl:31-34, 90-112
 * update_feature_maps!(rule::HALSUpdate, data, W, H; l1H=0, l2H=0) -> loss   src/algs/hals.jl:37-42, 121-154
 * on the same handle (the HALSUpdate constructor, hals.jl:18-28, needs nothing beyond cmf_create +
 * cmf_set_factors: the residual it carries is est - data, kept implicitly).  Same Gauss-Seidel visiting
 * order as the reference; clamp at 0 and "+ l2" regularisation as in hals.jl:110,153.
 * Unsharded handles only (the H sweep is sequential along T).  Any K, L the reference accepts runs: the fast on-chip
 * sweeps cover L <= 64 (H) and L * Kpad <= 2048, K * L <= 2048 (W; Kpad = K rounded up to 32); beyond them general sweeps
 * run the same recurrences in the same order with their state in LDS (slower; up to L * Kpad = 16384).
 * cmf_set_option(h, "hals_prepare", 1) allocates the rule's scratch at construction time instead of at the first update.
 * The H sweep normally runs as one persistent launch whose workgroups (a sweeper per row of H, puller workgroups that
 * apply the cross-row terms) wait for each other through flags in device memory.  It needs the device to itself for
 * those ~2 ms: every such wait is bounded (about two seconds), and if one runs out -- another process or stream holding
 * the CUs -- cmf_hals_update_feature_maps restores H from the snapshot taken at the start of the sweep, redoes the sweep
 * with one launch per pipeline stage (no co-residency needed; the handle keeps to that form afterwards) and returns
 * CMF_OK; cmf_get_counter(h, "hals_pipeline_reruns") counts these events.
 * cmf_set_option(h, "hals_persist", 0) selects the one-launch-per-stage pipeline from the start. */
int cmf_hals_update_motifs(cmf_handle h, double l1W, double l2W);
int cmf_hals_update_feature_maps(cmf_handle h, double l1H, double l2H, double *loss);

/* ---- PGD rule ------------------------------------------
 * update_motifs!(rule::PGDUpdate, data, W, H; loss_func=SquareLoss(), constrW, penaltiesW)      src/algs/pgd.jl:158-177
 * update_feature_maps!(rule::PGDUpdate, data, W, H; loss_func, constrH, penaltiesH) -> loss    src/algs/pgd.jl:180-202
 * with SquareLoss (pgd.jl:29-36) or AbsoluteLoss (pgd.jl:41-47; cmf_pgd_set_loss); pen_sq / pen_abs are the summed
 * weights of the SquarePenalty / AbsolutePenalty entries of the penalty list (pgd.jl:74-89); `constraint` selects
 * 0 = none, 1 = NonnegConstraint (max(eps, x), pgd.jl:92-96), 2 = UnitNormConstraint (every component k whose slice
 * W[k,:,:] / H[k,:] has norm > 1 is scaled to norm 1, pgd.jl:100-110).
 * The rule's state (stepW = stepH = 5, cur_loss = norm(data), step_incr 1.05, step_decr 0.70; pgd.jl:139-154)
 * lives in the handle and is (re)initialised by cmf_create and cmf_pgd_reset.  Valid on single-GPU handles and on group
 * handles (cmf_create_multi / cmf_comm_init_*): one all-reduce of the partial gradW per iteration; the squared norm of gradH,
 * the component norms of UnitNormConstraint and the loss are summed over the shards in rank order, the step-size state
 * machine is replicated (every rank takes the same accept / reject decisions). */
int cmf_pgd_reset(cmf_handle h);
/* MaskedLoss(SquareLoss(), mask)  src/algs/pgd.jl:58-70 (the loss_func of the reference's own test/test.jl:45):
 * gradient 2*(est - data) .* mask, loss norm(mask.*data - mask.*est)^2.  `mask` is N x T column-major like data
 * (borrowed for the call); NULL restores the plain SquareLoss.  The PGD entries read the mask as weights; the MU entries read it
 * only when it was installed with cmf_mu_set_mask (below), and run unmasked again after this call.  On a group handle the
 * mask is cut along T like data: cmf_create_multi groups take the whole N x T mask, a cmf_create_shard handle its own
 * columns followed by the right lag halo (the layout of data_local). */
int cmf_set_mask(cmf_handle h, const double *mask);
/* The MU rule under a mask: the multiplicative update (src/algs/mult.jl:23-58) of the weighted objective
 * norm(mask .* (data - tensor_conv(W, H)))^2 -- MaskedLoss (src/algs/pgd.jl:58-70) for the headline rule, so that entries of data
 * can be held out of a fit and scored afterwards (cmf_masked_loss).  `mask` is N x T column-major like data (borrowed for the
 * call), 0 and 1 only, 1 = observed; it goes into the handle's one mask (the storage of cmf_set_mask).  From then on
 * cmf_update_motifs, cmf_update_feature_maps, cmf_iterate, cmf_fit and cmf_compute_loss run mult.jl with
 * data -> Xm = select(mask, data, 0) and est -> mask .* est wherever the rule reads them.  A select, not a product: what data
 * holds under mask == 0 (NaN and Inf included: missing samples) never enters.
 * LOSS: norm(mask .* (est - data)) / norm(Xm) -- the share of the FITTED entries left unexplained.  pgd.jl:201 divides by
 * norm(data) for MaskedLoss; with missing samples that norm may be NaN, and the two agree for an all-ones mask.
 * A row or column without an observed entry is legal (its factor entries fall to eps, as the formulas say).
 * NULL restores the unmasked rule and frees the mask and the masked copies.  Every option is honoured under a mask except
 * "gram".  Errors: CMF_ERR_ARG for a mask that is not 0/1 or observes nothing; CMF_ERR_UNSUPPORTED with the Gram forms (option
 * "gram": the Gram rewriting of the denominators has no masked form) and on group handles (cmf_create_multi, cmf_create_shard);
 * the HALS entries answer CMF_ERR_STATE while this mask is installed. */
int cmf_mu_set_mask(cmf_handle h, const double *mask);
/* Sums over the entries with mask != 0 (complement != 0: over the entries with mask == 0) of (tensor_conv(W, H) - data)^2 and of
 * data^2, for the resident factors: sqrt(resid_sumsq / data_sumsq) is the masked loss (pgd.jl:58-70) on the observed entries,
 * or the held-out score on the others.  Both sums are by select, so a NaN among the held-out data never enters the observed sums.
 * One loss-only conv and one pass over data; est, the factors and the rule's state are left as they were.  Works with the mask of
 * cmf_mu_set_mask or of cmf_set_mask; CMF_ERR_STATE without one, CMF_ERR_UNSUPPORTED on group handles. */
int cmf_masked_loss(cmf_handle h, int complement, double *resid_sumsq, double *data_sumsq);
/* The divergence the MU rule minimises.  CMF_DIV_SQUARE (default) is src/algs/mult.jl as it stands and restores exactly today's rule,
 * launch for launch.  CMF_DIV_KL is the multiplicative update of the generalised Kullback-Leibler divergence (Smaragdis' convolutive
 * NMF; beta_loss="kullback-leibler" elsewhere), for counts and spectrogram magnitudes.  With eps = eps(Float64) (src/CMF.jl:20) and
 * e = tensor_conv(W, H) + eps, from this call on cmf_update_motifs, cmf_update_feature_maps, cmf_compute_loss, cmf_iterate and
 * cmf_fit (eval_mode included) run
 *   update_motifs!:        R = data ./ e;  numW[:, :, l] = shift_cols(H, l) * R[:, 1+l:T]'  (mult.jl:32 with data -> R);
 *                          denomW[k, n, l] = sum(H[k, 1:T-l])  (the same for every n; 0 when l >= T);
 *                          W .*= numW ./ (denomW + l1W + 2 l2W W + eps);  W = max(eps, W)  (mult.jl:37-38 unchanged)
 *   update_feature_maps!:  R = data ./ e (e from the new W);  numH = tensor_transconv(W, R);
 *                          denomH[k, t] = sum over l < min(L, T-t+1), over n, of W[k, n, l+1];  the same update of H
 * -- denomW and denomH are what mult.jl:33 and :48 give with est replaced by all ones.
 * LOSS: D(data, e) / sum(data), D = sum over entries of (data > 0 ? data log(data / e) : 0) - data + e, with e from the new H:
 * dimensionless, 0 for a perfect fit, no square root, and with l1 = l2 = 0 it does not increase from one iteration to the next.
 * Data must be finite and non-negative with a positive sum (checked here in one pass over the resident data); zeros are legal, and
 * so is a unit whose data are all zero (its motif entries fall to eps).  Every option is honoured except "gram"; the few-component
 * fusions that "small_k_fuse" and "speculate" select are not taken under KL, so results do not depend on them.
 * Errors: CMF_ERR_ARG for another kind, or for data with a negative, NaN or infinite entry or a sum of 0; CMF_ERR_UNSUPPORTED on
 * group handles (cmf_create_multi, cmf_create_shard), with the Gram forms (option "gram", in either order) and together with
 * cmf_mu_set_mask (in either order); the HALS and PGD entries answer CMF_ERR_STATE while CMF_DIV_KL is installed. */
#define CMF_DIV_SQUARE 0
#define CMF_DIV_KL 1
int cmf_mu_set_divergence(cmf_handle h, int kind);
/* The KL form under a mask: cmf_set_option(h, "kl_mask", 1) (default 0; values other than 0 and 1: CMF_ERR_ARG; cmf_option_names does
 * not list it, like "nnls_large" below).  With it on, cmf_mu_set_mask under CMF_DIV_KL and cmf_mu_set_divergence(CMF_DIV_KL) under
 * a mask both succeed, in either order, and the MU entries run, with M the mask and Xm = select(M, data, 0),
 *   update_motifs!:        R = Xm ./ e (exactly 0 where M == 0, whatever data holds there);  numW as above from this R;
 *                          denomW[:, :, l] = shift_cols(H, l) * M[:, 1+l:T]'  (mult.jl:33 with est -> M: no longer the same for every n)
 *   update_feature_maps!:  R from the new W;  numH = tensor_transconv(W, R);  denomH = tensor_transconv(W, M)
 * LOSS: D_M / sum(Xm), D_M the divergence terms summed over the entries with M == 1.  Data must be finite and non-negative WHERE
 * OBSERVED with sum(Xm) > 0: installing the second of the two checks Xm, and whatever takes the MU mask away while CMF_DIV_KL is
 * installed (cmf_mu_set_mask(h, NULL), cmf_set_mask) checks the raw data first -- CMF_ERR_ARG, and the handle as it was, when a
 * check fails.  A unit or a sample with nothing observed is legal (numerator and denominator are 0 there: its factor entries fall
 * to eps); with an all-ones mask the rule is the unmasked KL rule.  cmf_masked_loss then returns (sum of the divergence terms, sum
 * of data) over the selected entries.  Turning the option off while both are installed: CMF_ERR_STATE.  Off (the default), every
 * call answers as documented above: CMF_ERR_UNSUPPORTED for the combination.  Groups, the Gram forms, the HALS and PGD entries and
 * real-valued weights stay refused as above. */
/* The Itakura-Saito and beta forms (below) under a mask: cmf_set_option(h, "pq_mask", 1), exactly in the manner of "kl_mask" (default
 * 0; values other than 0 and 1: CMF_ERR_ARG; single-GPU handles only; cmf_option_names does not list it; turning it off while a
 * mask and CMF_DIV_IS or a beta-divergence are both installed: CMF_ERR_STATE).  With it on, mask and divergence may be installed
 * in either order and cleared in either order, and the MU entries run on
 *   Q = M .* e.^(beta - 1)  (Itakura-Saito: M ./ e),     P = M .* data .* e.^(beta - 2)  (Itakura-Saito: (data .* Q) .* Q where M == 1)
 * -- EXACT 0 in both arrays at the held-out entries, by a select: what data holds there (NaN, Inf, negatives) never enters -- with
 * the contractions, the exponents, the step exponent gamma and the loss terms of the unmasked form.  LOSS (update_feature_maps!,
 * cmf_compute_loss): the divergence terms summed over the entries with M == 1, divided by their number.  cmf_masked_loss then
 * returns (sum of the divergence terms, number of entries) over the selected entries; with `complement` the terms are taken on the
 * RAW data of the held-out entries, which no check has seen: a NaN there makes the sum NaN, and a value below 0 is left out of the
 * sum while the count still includes it (the epilogue reads "below 0" as "not selected") -- score held-out data that passes the
 * form's own check.  Data must pass the form's check WHERE
 * OBSERVED (Itakura-Saito: finite and > 0; beta: finite and >= 0): installing the second of the two checks it, and whatever takes
 * the MU mask away while the form is installed checks the raw data first -- CMF_ERR_ARG with the form's own text, and the handle as
 * it was, when a check fails.  A unit or a sample never observed is legal (both sums are 0: its factor entries fall to eps); with
 * an all-ones mask W and H are those of the unmasked form.  Every switch voids est, the speculated contraction and a deferred loss.
 * Off (the default), every call answers as documented: CMF_ERR_UNSUPPORTED for the combination.  Groups, the Gram forms and the
 * HALS and PGD entries stay refused. */
/* The HALS rule under a mask: cmf_set_option(h, "hals_mask", 1) (default 0; values other than 0 and 1: CMF_ERR_ARG; single-GPU
 * handles only; cmf_option_names does not list it, like "kl_mask" above).  With it on, and a 0/1 mask of cmf_mu_set_mask installed
 * under CMF_DIV_SQUARE, cmf_hals_update_motifs and cmf_hals_update_feature_maps run HALS BY IMPUTATION, the form seqNMF uses for
 * missing data: before each half-update the held-out entries of data are replaced by the current estimate,
 *   X~ = select(M, data, tensor_conv(W, H)),
 * and the ordinary half-update (src/algs/hals.jl) runs on X~.  X~ is never formed: the rule reads the residual only, and
 * est - X~ = M .* (est - data).  The convs store (est - Xm) .* M with Xm = select(M, data, 0), an exact 0 at a held-out entry whatever
 * data holds there (NaN and Inf included); G of the W half and P of the H half are contracted from it, the sweeps are unchanged.
 * Every step of a half-update minimises a block of norm(X~ - est)^2 exactly, and that majorises norm(M .* (data - est))^2 with
 * equality at the current point: with l1 = l2 = 0 the loss does not increase, and the fixed points are those of the masked objective.
 * LOSS: norm(M .* (est - data)) / norm(Xm), the masked MU rule's (cmf_mu_set_mask above), so the two rules' loss_hist compare.
 * "hals_gram": its difference forms (2, the default, and 1) would contract X~ itself; while this form runs both projections come
 * from the stored residual as under hals_gram = 0.  The stored value is kept and applies again when the mask or the option goes.
 * Every other HALS option is honoured ("hals_chase" included: the chasing tiles carry the masked epilogue).  With an all-ones mask W
 * and H are those of the plain rule under hals_gram = 0, bit for bit.  The option can be switched at any time; a switch voids est
 * and the speculated contraction.  Off (the default), the HALS entries answer CMF_ERR_STATE while the mask is installed, as
 * documented above.  Real-valued weights and the mask of cmf_set_mask stay the PGD rule's (the HALS entries ignore them); groups
 * and a divergence other than CMF_DIV_SQUARE stay refused.  cmf_get_counter "hals_masked_convs": conv launches with the masked
 * residual epilogue made by the HALS entries (0 while the form has not run). */
/* CMF_DIV_IS: the multiplicative update of the Itakura-Saito divergence (beta = 0; beta_loss="itakura-saito" elsewhere), the
 * scale-invariant objective for POWER spectrograms: a quiet harmonic weighs as much as a loud one.  It is taken by
 * cmf_mu_set_divergence only after cmf_set_option(h, "is_div", 1) (default 0; values other than 0 and 1: CMF_ERR_ARG; single-GPU
 * handles only; cmf_option_names does not list it, like "kl_mask" above; turning it off while CMF_DIV_IS is installed:
 * CMF_ERR_STATE).  With the option off every call answers as documented above, kind 2 with CMF_ERR_ARG.  With e as above,
 * Q = 1 ./ e and P = (data .* Q) .* Q, the MU entries run
 *   update_motifs!:        numW[:, :, l] = shift_cols(H, l) * P[:, 1+l:T]';  denomW[:, :, l] = shift_cols(H, l) * Q[:, 1+l:T]'
 *                          (mult.jl:32-33 with data -> P, est -> Q);
 *                          W .*= sqrt.(numW ./ (denomW + l1W + 2 l2W W + eps));  W = max(eps, W)
 *   update_feature_maps!:  P, Q from the new W;  numH = tensor_transconv(W, P);  denomH = tensor_transconv(W, Q);  the same
 *                          square-root update of H
 * -- the exponent 1/2 is the majorisation-minimisation step for beta < 1 (Fevotte & Idier 2011): with l1 = l2 = 0 the loss does not
 * increase.  LOSS: D / (N T), D = sum over entries of (r - 1) - log(r), r = data ./ e, with e from the new H: the mean divergence
 * per entry, dimensionless, unchanged when data and the estimate are scaled together, 0 for a perfect fit, no square root.
 * Data must be finite and STRICTLY positive (an exact zero has infinite divergence): checked in one pass when the divergence is
 * installed, CMF_ERR_ARG with a text that starts "Itakura-Saito divergence needs" -- add a small floor to the spectrogram.
 * Every option is honoured except "gram"; the few-component fusions are not taken, so results do not depend on "small_k_fuse",
 * "speculate" or "reuse_est".  CMF_ERR_UNSUPPORTED on group handles, with the Gram forms and together with cmf_mu_set_mask (in
 * either order: the form has no masked form); the HALS and PGD entries answer CMF_ERR_STATE while it is installed.  Switching
 * between the three kinds on one handle voids est, the speculated contraction and a deferred loss each time. */
#define CMF_DIV_IS 2
/* The beta-divergence between those three points (beta_loss=<float> elsewhere): beta = 0.5 is the usual compromise between
 * Itakura-Saito and KL for audio, 1 < beta < 2 the Tweedie compound-Poisson range, beta = 2 the squared error (halved).  With e as
 * above, Q = e.^(beta - 1) and P = data .* e.^(beta - 2), the MU entries run
 *   update_motifs!:        numW[:, :, l] = shift_cols(H, l) * P[:, 1+l:T]';  denomW[:, :, l] = shift_cols(H, l) * Q[:, 1+l:T]'
 *                          (mult.jl:32-33 with data -> P, est -> Q);
 *                          W .*= (numW ./ (denomW + l1W + 2 l2W W + eps)).^gamma;  W = max(eps, W)      (mult.jl:37-38)
 *   update_feature_maps!:  P, Q from the new W;  numH = tensor_transconv(W, P);  denomH = tensor_transconv(W, Q)  (mult.jl:47-48);
 *                          the same update of H (mult.jl:51-52)
 * with the majorisation-minimisation exponent gamma = 1 / (2 - beta) for beta < 1, 1 for 1 < beta <= 2 (the element-wise kernels of
 * the squared-error rule, untouched) and 1 / (beta - 1) for beta > 2 (Fevotte & Idier 2011): with l1 = l2 = 0 the loss does not
 * increase.  LOSS: D / (N T), D = sum over entries of d(x | e) = (x^beta + (beta - 1) e^beta - beta x e^(beta - 1)) / (beta (beta - 1))
 * with e from the new H: the mean divergence per entry, like CMF_DIV_IS (summed in a form that does not cancel: DESIGN.md 6a-beta).
 * ACCEPTED: CMF_BETA_WINDOW <= beta <= CMF_BETA_MAX with |beta - 1| >= CMF_BETA_WINDOW.  beta = 0 and beta = 1 are CMF_DIV_IS and
 * CMF_DIV_KL (the formula is 0/0 there; the text says so); beta < 0 takes e^(beta - 2) out of fp32; close to 0 and to 1 the factor
 * 1 / (beta (beta - 1)) takes the digits of the fp32 loss (profiles/mu_beta_precision.txt has the window); above 4, x^beta leaves
 * fp32 for entries of ordinary size.  All of these and a NaN: CMF_ERR_ARG, the handle as it was.
 * Data must be finite and non-negative (an exact zero is legal: its term is e^beta / beta): checked in one pass when the form is
 * installed, CMF_ERR_ARG with a text that starts "the beta-divergence needs".  Calling it again with another beta changes the
 * exponent and voids est.  cmf_mu_set_divergence(h, CMF_DIV_SQUARE / CMF_DIV_KL / CMF_DIV_IS) leaves the form (kind 3 is not a
 * kind: CMF_ERR_ARG); CMF_DIV_SQUARE restores the plain rule launch for launch.  Refusals as for CMF_DIV_IS: CMF_ERR_UNSUPPORTED on
 * group handles, with the Gram forms and together with cmf_mu_set_mask (in either order); the HALS and PGD entries answer
 * CMF_ERR_STATE while it is installed.  The few-component fusions are not taken, so results do not depend on "small_k_fuse",
 * "speculate" or "reuse_est". */
#define CMF_BETA_WINDOW 0.01
#define CMF_BETA_MAX 4.0
int cmf_mu_set_beta_divergence(cmf_handle h, double beta);
/* seqNMF's cross-orthogonality penalties (Mackevicius et al., eLife 2019) on the squared-error MU rule.  With
 *   S(A)[k,t]   = sum of A[k,t'] over |t' - t| <= L-1, 0 <= t' < T     (seqNMF's conv2(A, ones(1, 2L-1), 'same'))
 *   off(A)[k,:] = sum of A[k',:] over k' != k,    A = tensor_transconv(W, data) (the rule's numH),    G = off(S(H)),
 *   Wflat[k,n]  = sum_l W[k,n,l]
 * the objective is 1/2 |data - tensor_conv(W,H)|^2 + lambda sum_{i != j} (A S H')_ij + lambda_H / 2 sum_{i != j} (H S H')_ij
 * + lambda_W / 2 sum_{i != j} (Wflat' Wflat)_ij, and the MU entries run mult.jl:23-58 with each denominator enlarged BEFORE the
 * regularisers:
 *   update_motifs!:        xW[k,n,l] = sum_t G[k,t] data[n,t+l]  (the contraction of mult.jl:32 with G in H's place);  oW[k,n,l] = off(Wflat)[k,n];
 *                          denomW + (lambda xW + lambda_W oW) in place of denomW in mult.jl:37
 *   update_feature_maps!:  xH = off(S(numH)) (numH of the same call: from the new W);  oH = G (from the H being updated);
 *                          denomH + (lambda xH + lambda_H oH) in place of denomH in mult.jl:51
 * xW and xH are the exact gradients of the lambda term, oH and oW seqNMF's terms (the gradients of the halved sums).  Everything else
 * is the plain rule: the eps clamp, est recomputed with the new W, the loss norm(est - data) / norm(data) -- the penalties are
 * reported by cmf_mu_xortho_cost, not added to it.  The update is not guaranteed monotone (seqNMF's is not either).
 * All weights 0 (the default): the plain rule, launch for launch.  With any weight non-zero the few-component fusions and the
 * speculated contraction are not taken (results do not depend on "small_k_fuse" or "speculate"); est reuse stays; eval_mode works.
 * The weights are state of the handle: cmf_update_motifs / cmf_update_feature_maps, cmf_iterate and cmf_fit all see them; they
 * survive cmf_set_factors and are changed by this entry alone.  The HALS, PGD, ADMM, ANLS and separable entries ignore them.
 * CMF_ERR_ARG for a negative, NaN or infinite weight.  CMF_ERR_UNSUPPORTED for non-zero weights on a group handle, under a mask
 * of cmf_mu_set_mask, under a divergence other than CMF_DIV_SQUARE or with the Gram forms -- and for installing any of those while a
 * weight is non-zero.  cmf_get_counter "xortho_launches" counts the launches of the penalties' own kernels. */
int cmf_mu_set_xortho(cmf_handle h, double lambda_xortho, double lambda_ortho_H, double lambda_ortho_W);
/* The three penalty sums of the resident factors WITHOUT their weights and without the 1/2, summed in fp64:
 * *xortho = sum_{i != j} (A S H')_ij,  *ortho_H = sum_{i != j} (H S H')_ij,  *ortho_W = sum_{i != j} (Wflat' Wflat)_ij.  Any pointer
 * may be NULL.  Costs one one-source transconv of data (mult.jl:47) plus the small kernels.  Single-GPU handles only. */
int cmf_mu_xortho_cost(cmf_handle h, double *xortho, double *ortho_H, double *ortho_W);
/* The four unweighted denominator terms above for the resident factors: xW and oW in the shape of W (K x N x L), xH and oH in the
 * shape of H (K x T), Julia memory order.  Any pointer may be NULL.  They show which component pairs the penalty acts on (what
 * mult.jl:37 and :51 get added to their denominators is lambda xW + lambda_W oW and lambda xH + lambda_H oH).  Single-GPU handles only. */
int cmf_mu_xortho_terms(cmf_handle h, double *xW, double *xH, double *oH, double *oW);
/* ---- seqNMF's significance test of components on held-out data (test_significance.m) ----
 * The test asks of each component k whether the overlap of its motif with held-out data, tensor_transconv(W, X)[k, :] (common.jl:71-81),
 * is more right-skewed than the overlaps of null motifs, whose rows are circularly shifted along the lag axis (seqNMF's
 * circshift(W(n, k, :), s)) by an amount of their own per (draw, component, unit):  draw 0 is the identity, and for d >= 1
 *   s(d, k, n) = ((bits(base(seed, 0x5157), ((d - 1) K + k) N + n) >> 32) * L) >> 32     in 64-bit integer arithmetic,
 * base and bits those of the library's counter generator (the one of cmf_init_rand / cmf_gen_synthetic: model.jl:113-125).
 * cmf_null_shifts writes that table for draws first_draw ... first_draw + n_draws - 1 as an (N, K, n_draws) array, n fastest.  Host only:
 * no device, no handle.  CMF_ERR_ARG: shifts NULL, n_draws < 1, first_draw < 0, K, N or L < 1, L > 4096. */
int cmf_null_shifts(uint64_t seed, int64_t first_draw, int64_t n_draws, int64_t K, int64_t N, int64_t L, int32_t *shifts);
/* The raw power sums of the overlaps of the null motifs of the handle's resident W with the handle's raw data (the held-out columns the
 * handle was created from):  with Wnull_d[k, n, l] = W[k, n, (l - s(d, k, n)) mod L] and v_d = tensor_transconv(Wnull_d, data)
 * (common.jl:71-81: terms with t + l > T are dropped; seqNMF's helper wraps circularly instead, which is the same on data followed by L
 * zero columns),  sums[0..2, k, j] = sum_t v, sum_t v^2, sum_t v^3 of draw first_draw + j, a (3, K, n_draws) column-major array of
 * doubles.  v is the fp32 contraction, widened to fp64 before it is squared and cubed; the sums are fp64 in a fixed order, so a draw's
 * result is a function of (W, data, seed, d) alone: bitwise the same whatever the batch size (cmf_set_option "signif_batch": draws per
 * batch, not listed by cmf_option_names; 0 = the default, the smallest multiple of 32 / gcd(K, 32) draws that fills 8 column blocks of
 * 32), however a range of draws is cut into calls, and whatever CU count the handle is planned for.  The skewness, the p-values and the
 * decision are host arithmetic on these sums (host.py: evaluate_significance).  The call reads the data and W and writes scratch of
 * its own (allocated on first use): est, a speculated contraction, a deferred loss, the slabs and the penalties' tables stay as they
 * are, and a fit continued after it gives the bits it gives without it.  cmf_get_counter "signif_launches" counts its kernels' launches.
 * CMF_ERR_ARG: NULL pointers, n_draws < 1, first_draw < 0.  CMF_ERR_STATE: factors not set; a mask installed (cmf_mu_set_mask /
 * cmf_set_mask: held-out entries of the data may hold NaN).  CMF_ERR_UNSUPPORTED: group and shard handles.  All before any device work. */
int cmf_null_moments(cmf_handle h, uint64_t seed, int64_t first_draw, int64_t n_draws, double *sums);
/* ---- seqNMF's re-centring of motifs (shiftFactors.m) ----
 * A convolutive factorisation does not change when motif k moves by s lags and row k of H by -s columns, so an MU fit can drift until a
 * motif straddles the edge of the L-lag window.  One step moves every motif's centre of mass back to the middle.  In 0-based lags,
 * for component k:  c_l = sum_n W[k,n,l] (n ascending),  m0 = sum_l c_l,  m1 = sum_l (l+1) c_l (lags ascending; all fp64, no fused
 * multiply-add),  c = max(floor(m1 / m0), 1),  centre = max(floor(L / 2), 1),  s_k = centre - c;  s_k = 0 where L == 1, where m0 is zero
 * or m0, m1 are not finite, and where the component is dead (no entry of W[k] above the MU clamp floor eps(Float64));  c is capped at
 * 2^30.  Then W'[k,n,l] = W[k,n,l-s_k] where 0 <= l-s_k < L and H'[k,t] = H[k,t+s_k] where 0 <= t+s_k < T; every vacated entry
 * takes the clamp floor (not 0: the MU rule cannot leave a zero).  Unlike seqNMF, H is shifted with fill, not circularly: the
 * convolutions here truncate at the ends of the recording.
 * cmf_recentre_shifts returns the K shifts of that definition for a K x N x L fp64 W in Julia's memory order.  Host only: no device,
 * no handle.  CMF_ERR_ARG: NULL pointers, K, N or L < 1. */
int cmf_recentre_shifts(const double *W, int64_t K, int64_t N, int64_t L, int32_t *shifts);
/* One step on the resident factors of a single-GPU handle, whatever rule produced them; the K shifts into `shifts` unless it is NULL
 * (the call synchronises only to return them).  What est holds is void afterwards.  CMF_ERR_STATE without factors,
 * CMF_ERR_UNSUPPORTED on group, front and shard handles (a shift of H crosses shard borders); both before any device work. */
int cmf_recentre(cmf_handle h, int32_t *shifts);
/* on = 1: the MU entries make that step in every update_feature_maps!, between the element-wise update of H (mult.jl:51-52) and the
 * loss conv (mult.jl:55-57) -- seqNMF's cycle: H update, shift, W update, cost.  It costs no contraction: est and the returned loss are
 * those of the shifted factors, est reuse and the speculated contraction stay valid, an armed write-back delivers the shifted W and H.
 * The step runs on the device inside the iteration (four small launches; no synchronisation, no copy to the host: a cmf_iterate
 * batch stays as pipelined as without it), and a step whose shifts are all zero moves no data and leaves W and H bitwise untouched.
 * With eval_mode (cmf_iterate, cmf_fit: W held fixed) nothing is shifted.  It runs under every form of the MU rule a single handle
 * takes but the Gram forms (their tables of W span the H phase): CMF_ERR_UNSUPPORTED for on = 1 with option "gram" set and for setting
 * "gram" while it is on.  State of the handle like the weights of cmf_mu_set_xortho: seen by cmf_update_feature_maps, cmf_iterate and
 * cmf_fit, it survives cmf_set_factors; the HALS, PGD, ADMM, ANLS and separable entries ignore it.  0 (the default): today's path,
 * launch for launch -- nothing allocated, nothing launched.  CMF_ERR_ARG for on outside 0 / 1, CMF_ERR_UNSUPPORTED on group, front and
 * shard handles.  cmf_get_counter "recentre_launches" counts the launches of the step's kernels. */
int cmf_mu_set_recentre(cmf_handle h, int on);
/* The K shifts of the most recent step (cmf_recentre or an MU entry) and the per-component totals of |s_k| since the handle was made;
 * zeros before the first step.  Either pointer may be NULL.  Synchronises.  CMF_ERR_UNSUPPORTED on group, front and shard handles. */
int cmf_mu_recentre_info(cmf_handle h, int32_t *last_shifts, int64_t *moved);
/* loss_func of the PGD entries: 0 = SquareLoss (default), 1 = AbsoluteLoss (gradient sign(est - data), loss
 * norm(data - est, 1); pgd.jl:41-47).  Combines with cmf_set_mask as MaskedLoss(loss, mask).
 * ACCURACY: with AbsoluteLoss the factors are held to 3e-4 (Frobenius-relative against the fp64 reference arithmetic), not
 * the 1e-4 of every other rule and loss: the gradient is sign(est - data), and an entry of est within fp32 rounding of
 * data takes the other sign than in fp64 -- a discontinuity no fp32 path can follow.  loss_hist stays within 1e-4. */
int cmf_pgd_set_loss(cmf_handle h, int loss_kind);
int cmf_pgd_update_motifs(cmf_handle h, double pen_sq, double pen_abs, int constraint);
int cmf_pgd_update_feature_maps(cmf_handle h, double pen_sq, double pen_abs, int constraint, double *loss);
int cmf_pgd_get_steps(cmf_handle h, double *stepW, double *stepH);

/* ---- ADMM rule ----------------------------------------------------------------------------------------------------------
 * The fourth rule of the reference (src/CMF.jl:4), computed in fp64 end to end: data, factors, auxiliaries, contractions, the
 * Gram matrices, their factorisations and the FFT ("The ADMM rule", says why and how).  The entries take the caller's
 * arrays in and out -- the rule reads exactly what it is handed and overwrites the other factor in place, as the reference does --
 * and keep clear of cmf_set_factors / cmf_arm_writeback, whose device copies are fp32.  Single-GPU handles only: a handle that
 * fronts a T-sharded group gets CMF_ERR_UNSUPPORTED.  cmf_get_counter "admm_W_reverts" / "admm_H_reverts" give the reverts
 * (admm.jl:101-105, :205-209) of the last call of each kind.
 *
 * ADMMUpdate(data, W, H) (src/algs/admm.jl:13-21): uploads `data` (N x T, fp64) and keeps norm(data); allocates the rule's fp64
 * state on the handle's device.  The random U of the constructor is zeroed before every use (admm.jl:46-48) and is not kept. */
int cmf_admm_prepare(cmf_handle h, const double *data);
/* update_motifs!(rule::ADMMUpdate, data, W, H; rhow=10, admm_W_maxiter=30, admm_tol=1e-4, nonnegW=true)  src/algs/admm.jl:24-121.
 * Reads H (K x T) only and overwrites W (K x N x L) with the fold of Z3 (admm.jl:114-120).  G = Hstk*Hstk' + 2I (admm.jl:53) is
 * factorised once per call; the inner loop (admm.jl:61-108) starts from zero auxiliaries and duals, updates the duals before the
 * loss, and reverts Z3 / breaks on the loss history of the call.  *iters (may be NULL) receives the inner iterations run.
 * L*K <= 8192. */
int cmf_admm_update_motifs(cmf_handle h, const double *H, double *W, double rhow, int64_t maxiter, double tol, int nonnegW,
                           int64_t *iters);
/* update_feature_maps!(rule::ADMMUpdate, data, W, H; rhoh=10, admm_H_maxiter=30, l1H=0, admm_tol=1e-4, nonnegH=true) -> loss
 * src/algs/admm.jl:124-226.  Reads W only and overwrites H with Z3 (admm.jl:219); *loss = norm(conv(W, H) - data) / norm(data)
 * (admm.jl:225).  The linear solve uses rho = 1 whatever rhoh is (precompute_solveH(W, 1, T), admm.jl:167, 180-182); the Z1 step
 * uses the circular convolution (tesnor_circconv!, common.jl:36-50), the loss the linear one; the revert / break check comes
 * before the dual update (admm.jl:203-216).  Needs T >= L (CMF_ERR_ARG: the reference indexes wh[:, :, 1:L], admm.jl:233) and
 * K <= 64 (CMF_ERR_UNSUPPORTED).  *iters (may be NULL) receives the inner iterations run. */
int cmf_admm_update_feature_maps(cmf_handle h, const double *W, double *H, double rhoh, int64_t maxiter, double l1H, double tol,
                                 int nonnegH, double *loss, int64_t *iters);

/* ---- ANLS rule ----------------------------------------------------------------------------------------------------------
 * Alternating non-negative least squares (src/algs/anls.jl), computed in fp64 end to end, restated on the K x N x L layout of W
 * (anls.jl is written for the old L x N x K one): every half step is the exact minimiser of its block.  The NNLS solver is block
 * principal pivoting on the normal equations with tol = 1e-5 (NNLS_TOL, anls.jl:18), which stands for nonneg_lsq(...; alg=:pivot)
 * of the reference; DESIGN.md, "The ANLS rule", says what is assumed about that package.  Like the ADMM entries these take the
 * caller's arrays in and out -- each call reads the factor the reference reads and overwrites the other in place -- keep nothing
 * of the factors on the device between calls, and stay clear of cmf_set_factors / cmf_arm_writeback.  Single-GPU handles only: a
 * handle that fronts a T-sharded group gets CMF_ERR_UNSUPPORTED.
 *
 * A problem whose passive-set Gram is not positive definite (rank-deficient or non-finite input), or that reaches the cap on
 * pivoting rounds (5 n + 10 for n unknowns; 50 n + 50 under "anls_backup_only"), ends the call with CMF_ERR_UNSUPPORTED and a
 * message; the caller's output factor is then untouched.  An all-zero stacked row of H or component of W is no such case: its
 * unknowns stay zero.
 *
 * cmf_set_option(h, "anls_backup_only", 1): every exchange of every problem moves only the infeasible index of largest number
 * (the solver's backup rule, i.e. plain principal pivoting): the same answer in more rounds.  It is the rule's only option and
 * exists so that a test can walk the backup path; it selects no path of the other rules and cmf_option_names does not list it.
 * cmf_get_counter: "anls_W_exchanges" / "anls_H_exchanges" = pivoting rounds summed over the problems of the last call of that
 * kind; "anls_backup" = problems of the last call that took the backup rule; "anls_capped" = problems of the last call that hit
 * the cap.
 *
 * cmf_set_option(h, "nnls_large", 1) (default 0; cmf_option_names does not list it either): cmf_anls_update_motifs and
 * cmf_sep_nnls solve problems of 129 .. 1024 unknowns, which they otherwise refuse, with the same solver -- the same exchange
 * rules, cap, tol, counters and failure behaviour -- whose factorisation runs blocked through device scratch (persistent
 * workgroups, one slab each; csrc/cmf_nnls_large.h).  The scratch is allocated by the first call that needs it and freed with
 * the handle's state; if it cannot be allocated the call returns CMF_ERR_HIP.  Problems of up to 128 unknowns run as with 0, bit
 * for bit.  Single-GPU handles only; any value but 0 or 1 is CMF_ERR_ARG.
 *
 * ANLSUpdate(data, W, H) (src/algs/anls.jl:10-14): uploads `data` (N x T, fp64) and keeps norm(data); allocates the rule's fp64
 * state on the handle's device.  (The residual the constructor forms is recomputed by every update_feature_maps!, anls.jl:27.) */
int cmf_anls_prepare(cmf_handle h, const double *data);
/* update_motifs!(rule::ANLSUpdate, data, W, H)  src/algs/anls.jl:22-24, :47-57.  Reads H (K x T) only and overwrites W (K x N x L)
 * with argmin_{W >= 0} |data - conv(W, H)|: N independent problems of K*L unknowns on G = Hstk*Hstk', C = Hstk*data', one
 * workgroup each, the passive-set Gram factorised in LDS.  K*L <= 128 (CMF_ERR_UNSUPPORTED beyond), or K*L <= 1024 under the option
 * "nnls_large" (above), where 129 and more unknowns are factorised through global scratch. */
int cmf_anls_update_motifs(cmf_handle h, const double *H, double *W);
/* update_feature_maps!(rule::ANLSUpdate, data, W, H; variant=:basic) -> loss  src/algs/anls.jl:26-36, :63-137.  Reads W and H,
 * overwrites H; *loss (may be NULL) = norm(conv(W, H) - data) / norm(data) of the new H (anls.jl:35).  variant 0 (:basic,
 * anls.jl:63-94): the columns t = 1..T in order, each the exact minimiser over H[:, t] >= 0 given the others -- one workgroup
 * walks T.  variant 1 (:block, anls.jl:101-137): L phases of columns l, l+L, ... <= T-L+1 solved side by side, then the last L-1
 * columns in order; needs T >= L (CMF_ERR_ARG: the reference indexes T-L+2:T).  Any other variant is CMF_ERR_ARG.  K <= 64 and
 * (L-1)*K <= 6144 (CMF_ERR_UNSUPPORTED). */
int cmf_anls_update_feature_maps(cmf_handle h, const double *W, double *H, int variant, double *loss);

/* ---- separable fit ---------------------------------------------------------------------------------------------------------
 * The "LCS" fit of src/algs/separable.jl (Separable.fit, separable.jl:14-56): successive projection, one NNLS, shift clustering.
 * It has no iteration; it is what the reference's notebooks start the other rules from.  Computed in fp64 end to end, restated on
 * the K x N x L layout of W (W[k, n, l] = V[n, groups[k][l]]); DESIGN.md 6d has the rewritings.  One entry per stage, so that a
 * caller (or a test) can run and inspect them one at a time; the decisions on R x R numbers between them (find_groups,
 * find_groups_spectral, sort_group, separable.jl:96-131, :191-270) and the eigen-decomposition behind `pre` are the host
 * language's.  Indices are 0-based.  Arrays are Julia's (column-major).  Single-GPU handles only, and the handle's K, L give
 * R = K*L where an entry does not take it.  cmf_get_counter: "sep_nnls_exchanges" = pivoting rounds of the last cmf_sep_nnls,
 * summed over its T problems.
 *
 * Uploads `data` (N x T, fp64) and allocates the state of the fit on the handle's device (separable.jl:19). */
int cmf_sep_prepare(cmf_handle h, const double *data);
/* X X' (N x N) of the matrix SPA works on -- the columns of data scaled to l1-norm 1, the ones with col1 < thresh zeroed
 * (separable.jl:281-291) -- for pre_svd / pre_svdcond (separable.jl:323-333): its eigen-decomposition gives the caller U and S. */
int cmf_sep_gram(cmf_handle h, double thresh, double *XXt);
/* SPA(data, R; thresh, pre) -> vertices (R of them, sorted)  separable.jl:280-319, with findsetmax (separable.jl:403-419) and the
 * col2 tie-break (:306-311) on the device; nothing is read back before all R rounds are enqueued.  pre 0: none; 1 (:svd) or 2
 * (:svdcond): `proj` holds R rows of N numbers, the matrix that takes X to Diagonal(S) * Vt = U' X or to Vt = S^-1 U' X
 * (row r at proj + r*N), else NULL.  1 <= R <= min(N, T) (CMF_ERR_ARG); N <= 4096; a residual that vanishes before R rounds
 * (fewer than R independent columns) is CMF_ERR_UNSUPPORTED. */
int cmf_sep_spa(cmf_handle h, int64_t R, double thresh, int pre, const double *proj, int64_t *vertices);
/* V = data[:, vertices]; G = nonneg_lsq(V, data); renormalize!(V, G)  separable.jl:23-27, :340-348.  V: N x R, G: R x T.  The T
 * problems share V'V and run in the solver of cmf_anls_update_motifs (tol 1e-8): R <= 128 (CMF_ERR_UNSUPPORTED beyond; R <= 1024
 * under the option "nnls_large" of the ANLS rule), the same
 * refusal of a non-positive pivot or a capped problem, V and G untouched on failure.  `vertices` is read only. */
int cmf_sep_nnls(cmf_handle h, int64_t *vertices, int64_t R, double *V, double *G);
/* What shift_cos / cosL (separable.jl:364-385) are made of, for shift_cluster (:144-150) and sort_group (:100-105):
 * P[a, b, l] = sum_t G[a, t] G[b, t+l] (R x R x L) and head[a, l] = norm(G[a, 1:T-l]) (R x L), so that
 * cosL(a, b, l, "a") = P[a, b, l] / (head[a, l] head[b, 0]) and cosL(a, b, l, "b") = P[b, a, l] / (head[a, 0] head[b, l]).
 * A zero row of G (a cosine 0/0) is CMF_ERR_UNSUPPORTED and the message names it; 1 <= L <= T. */
int cmf_sep_shift_table(cmf_handle h, const double *G, int64_t R, int64_t L, double *P, double *head);
/* construct_WH(V, G, groups; average_H=true)  separable.jl:59-87, with the reference's divisor min(T, t+L) - t + 1.  groups: K x L
 * rows of G (read only), in the sorted order; W: K x N x L, H: K x T. */
int cmf_sep_construct(cmf_handle h, const double *V, const double *G, int64_t *groups, double *W, double *H);

/* converged(loss_hist, patience, tol): src/model.jl:91-107 (host arithmetic). */
int cmf_converged(const double *loss_hist, int64_t len, int64_t patience, double tol);

/* ---- stand-alone primitives ------------------------------------------------
 * tensor_conv(W, H) -> est (N x T): src/common.jl:17-34. */
int cmf_tensor_conv(int device, int64_t N, int64_t T, int64_t K, int64_t L,
                    const double *W, const double *H, double *est);
/* tensor_transconv(W, X) -> out (K x T): src/common.jl:62-81. */
int cmf_tensor_transconv(int device, int64_t N, int64_t T, int64_t K, int64_t L,
                         const double *W, const double *X, double *out);

/* ---- the KL form of the MU rule on an event list ----------------------------
 * For counts that are mostly zeros (binned spikes, photon counts): data is given as its non-zero entries, events
 * (unit[j], time[j], count[j]) with data[unit[j], time[j]] = count[j], and the rule of cmf_mu_set_divergence with CMF_DIV_KL above runs
 * with every sum over the data taken over the events only.  The semantics are that rule's, unchanged (src/algs/mult.jl:23-58 with
 * data -> R; eps = eps(Float64), src/CMF.jl:20; the denominator and the clamp of mult.jl:37-38 and :51-52): R = data ./ e is zero where
 * data is zero, so with e_j = sum over l <= min(L-1, t_j), over k, of W[k, n_j, l] H[k, t_j - l] + eps and r_j = x_j / e_j
 *   update_motifs!:        numW[k, n, l] = sum over the events of unit n with t_j >= l of r_j H[k, t_j - l];  denomW as in the dense rule
 *   update_feature_maps!:  r_j from the new W;  numH[k, t] = sum over the events with t <= t_j <= t + L - 1 of W[k, n_j, t_j - t] r_j;
 *                          denomH as in the dense rule
 *   LOSS:                  (sum_j x_j log(x_j / e_j) - sum_j x_j + sum_all e) / sum_j x_j  with e from the new W and H, where
 *                          sum_all e = sum_k sum_{l < min(L, T)} (sum_n W[k, n, l]) (sum_{t < T - l} H[k, t]) + N T eps  (a closed form:
 *                          the sum of e over ALL N T entries, without forming them); event sums and the closed form are added in fp64,
 *                          in a fixed order
 * The cost of an iteration is O(nnz K L + K T L + K N L) and the handle holds O(nnz + K T + K N L) bytes: nothing of size N x T is ever
 * allocated (cmf_events_get_counter "device_bytes").  r_j and the log term are computed by the dense rule's own device functions, so
 * the two paths differ only in the order in which e is summed.  No float atomics: a unit or a column window with more events than
 * "unit_chunk" / "time_chunk" is cut into chunks whose partial sums are added in chunk order, so results are reproducible bit for bit.
 * One GPU; no mask, no other divergence, no T sharding, no Gram form, no cmf_arm_writeback. */
typedef struct cmf_events_s *cmf_events;
/* Events must be sorted by (unit, time), strictly increasing (so: no duplicates), with 0 <= unit < N, 0 <= time < T and counts that are
 * finite and > 0 (in their fp32 rounding too).  A unit or a time column without events is legal: its factor entries fall to eps, as
 * in the dense rule.  Errors, all raised BEFORE anything touches a device: CMF_ERR_ARG for N, T, K or L < 1, nnz < 1, a NULL
 * pointer, an index out of range, a count that is not finite and positive, or events out of order; CMF_ERR_UNSUPPORTED (the message names
 * the limit) for K > 256 or 32 * ceil(K / 32) * L > 4096 -- the kernels keep W[:, n, :] of one unit in LDS --, for nnz >= 2^31 and for
 * sizes the dense cmf_create refuses.  The arrays are copied: the handle keeps the events twice, unit-major and time-major (a stable
 * counting sort) with the permutation between the two. */
int cmf_events_create(cmf_events *h, int device, int64_t N, int64_t T, int64_t K, int64_t L,
                      int64_t nnz, const int32_t *unit, const int32_t *time, const double *count);
int cmf_events_destroy(cmf_events h);
/* W (K x N x L) and H (K x T) in Julia order, like cmf_set_factors and cmf_get_factors (get: either pointer may be NULL). */
int cmf_events_set_factors(cmf_events h, const double *W, const double *H);
int cmf_events_get_factors(cmf_events h, double *W, double *H);
/* update_motifs! (mult.jl:23-39) and update_feature_maps! (mult.jl:42-58; *loss receives the loss from the new W and H) in the event
 * form above; cmf_events_compute_loss is the loss of the resident factors (alternating.jl:37). */
int cmf_events_update_motifs(cmf_events h, double l1W, double l2W);
int cmf_events_update_feature_maps(cmf_events h, double l1H, double l2H, double *loss);
int cmf_events_compute_loss(cmf_events h, double *loss);
/* n_iter iterations of alternating.jl:45-60 (eval_mode != 0: update_motifs! is skipped, :51-53) without a host round trip per call;
 * loss_hist (n_iter values, may be NULL) is written at the end.  Bit for bit what the two rule calls give. */
int cmf_events_iterate(cmf_events h, int64_t n_iter, int eval_mode, double l1W, double l2W, double l1H, double l2H, double *loss_hist);
/* The terms of both updates for the resident W and H, element by element (tests): ratio[j] = r_j (nnz values, input order), numW and
 * denomW (K x N x L), numH and denomH (K x T), Julia order, each the fp32 value the update kernels read.  Any pointer may be NULL. */
int cmf_events_terms(cmf_events h, double *ratio, double *numW, double *numH, double *denomW, double *denomH);
/* Options: "unit_chunk" (default 128) and "time_chunk" (default 2048): the most events one workgroup sums for a unit (numW, the ratio)
 * and for a column's window (numH), values >= 1 -- the work tables are rebuilt; a small value on a long list costs one slab per chunk.
 * "keep_ratio" (default 1): update_motifs! reads the r_j the loss pass before it left, the way the dense rule keeps R; 0 computes them
 * again -- the results are bitwise the same.  CMF_ERR_ARG for another name or value. */
int cmf_events_set_option(cmf_events h, const char *name, int value);
/* Counters: "device_bytes" (everything the handle holds on the device), "launches" (kernel launches so far), "ratio_passes", "nnz",
 * "unit_chunk", "time_chunk", "keep_ratio", "unit_items" / "time_items" (workgroups of the two work tables), "unit_split" /
 * "time_split" (destinations cut into several chunks), "w_block_units" / "h_block_columns" (units and columns one workgroup of the
 * element-wise updates owns), "ratio_waves" (events a workgroup of the ratio pass has in flight). */
int cmf_events_get_counter(cmf_events h, const char *name, int64_t *value);

/* ---- initialisation / synthetic inputs -------------------------------------
 * init_rand(data, L, K): src/model.jl:113-125, with a portable counter-based
 * RNG in place of Julia's MersenneTwister (seed: fit_cnmf's `seed` kwarg,
 * src/model.jl:64-67).  Writes W (K x N x L), H (K x T). */
int cmf_init_rand(int device, int64_t N, int64_t T, int64_t K, int64_t L, uint64_t seed,
                  const double *data, double *W, double *H);
/* gen_synthetic (README.md:14) following synthetic_sequences
 * (datasets/synthetic.jl:29-61).  Writes data (N x T) and, when non-NULL,
 * the ground-truth W (K x N x L) and H (K x T). */
int cmf_gen_synthetic(int device, int64_t N, int64_t T, int64_t K, int64_t L,
                      double alpha, double p_h, double sigma, double noise_scale, uint64_t seed,
                      double *data, double *W, double *H);

/* ---- measurement hooks (bench.py) ------------------------------------------
 * Times `reps` launches of one named hot kernel with HIP events on the
 * handle's stream and returns the average duration in milliseconds plus the
 * algorithmic flop count of one launch.  name: "conv", "conv_t", "conv_loss", "conv_loss_store", "hxt", "transconv";
 * "signif_draw" (one default batch of cmf_null_moments, per DRAW) and "transconv1_sum" (the one-source transconv plus its slab sum).
 * On a group handle "allreduce" times the group's bulk exchange alone (the buffer an iteration all-reduces); it is a
 * collective -- every rank of the group makes the call -- and *flops receives the payload in bytes. */
int cmf_time_kernel(cmf_handle h, const char *name, int reps, double *avg_ms, double *flops);
/* In-loop timing: after cmf_set_option(h, "profile", 1) every contraction launch of the update / loss entries is
 * bracketed by a HIP event pair on the launch stream; cmf_kernel_times synchronises and returns the mean duration
 * and the number of launches recorded for one class: "conv" (mult.jl:28), "conv_t" (:44), "conv_loss" /
 * "conv_loss_store" (:55-57), "hxt" (:31-34; "hxt_num" / "hxt_den" for the one-source launches of the overlap and
 * Gram forms), "transconv" (:47-48).  Setting the option again restarts it; a value
 * n > 1 brackets only every n-th launch of each class (an event pair costs a few microseconds on the stream). */
int cmf_kernel_times(cmf_handle h, const char *name, double *avg_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* CMF_HIP_H */
