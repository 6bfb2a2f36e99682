/*
 * allred.h — C-ABI of the MI355X allreduce engine (liballred.so).
 *
 * Drop-in boundary for the reference EngineerCharlie/TenstorrentAllreduce.
 * Plain pointers and sizes only; every entry point names the reference
 * interface it replaces (file:line under the reference tree).  All functions
 * return ALLRED_OK (0) or a negative ALLRED_ERR_* code unless documented
 * otherwise; the reference itself has no error codes (bad configurations hang
 * the Wormhole) — here they are rejected up front.
 *
 * Host-only entry points (schedule, data generation, validation) never touch
 * the GPU.  Device entry points take a hipStream_t as `void* stream`
 * (NULL = the default stream) and enqueue asynchronously.
 */
#ifndef ALLRED_H
#define ALLRED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 7 (round 6): the one-deep peer pipeline (allred_peer_allreduce_pipelined, k_hier_x) and
 * k_hier_ll are retired, allred_peer_set_hier_ll takes 0 (launch form) / 1 (k_hier_ws, the
 * default), the tune keys hier_x2_tail / hier_x_lag / hier_x_chunked / hier_x_rearly /
 * hier_x_latepoll are gone (k_hier_x2 runs its measured product form only), and
 * allred_last_launch is new.  ABI 6 (round 5): the hierarchical forms' hand-off area holds
 * 6 data bytes + a 16-bit epoch per word — peers of different ABIs must not connect.
 * Still ABI 7: allred_run_io, allred_validate_device and allred_rank_check are additions —
 * no existing struct layout, signature or behaviour changes, so the version stays.
 * Still ABI 7: allred_plan_reduce_scatter / allred_plan_all_gather and allred_dist_reduce_scatter /
 * allred_dist_all_gather (+ their _host twins) are additions too — the two halves of the BO
 * allreduce as calls of their own, on the existing plans, descs and communicators.
 * Still ABI 7: allred_bucket and allred_plan_execute_group / allred_plan_reduce_scatter_group /
 * allred_plan_group_launches are additions — a list of buckets, the small ones sharing launches.
 * Still ABI 7: allred_shard_bucket and allred_plan_reduce_scatter_shards / allred_plan_all_gather_shards /
 * allred_plan_shards_launches are additions — the grouped reduce-scatter into, and the grouped
 * all-gather from, per-bucket shard buffers.
 * Still ABI 7: allred_shard_bucket_f32, ALLRED_SHARD_ACCUMULATE and allred_plan_reduce_scatter_shards_f32 /
 * allred_plan_all_gather_shards_f32 / allred_plan_shards_f32_launches are additions — the same two
 * calls on fp32 shards: the tree accumulated in fp32, one rounding to bf16 on the way back.
 * Still ABI 7: allred_plan_reduce_scatter_shards_f32_norm and allred_plan_shards_f32_norm_workspace_bytes
 * are additions — the fp32 grouped reduce-scatter that also leaves the per-rank squared gradient
 * norm of what it stored, in the same launch.
 * Still ABI 7: allred_adamw_bucket_f32, allred_adamw_hyper, ALLRED_ADAMW_GROUP_MAX, ALLRED_ADAMW_ZERO_GRAD and
 * allred_plan_adamw_all_gather_shards_f32 / allred_plan_adamw_shards_f32_launches are additions — the
 * clipped AdamW step on the fp32 shards inside the grouped all-gather's launch.
 * Still ABI 7: ALLRED_ADAMW_PARAM_GROUPS_MAX and allred_plan_adamw_all_gather_shards_f32_groups are additions —
 * the same step with a hyperparameter set per parameter group, chosen per bucket, in the same launches.
 * Still ABI 7: allred_mx_bucket_f32, ALLRED_MX_GROUP_MAX, ALLRED_MX_SCALE_RCEIL and
 * allred_plan_all_gather_shards_mxfp8 / allred_plan_all_gather_shards_mxfp8_launches are additions — the grouped
 * all-gather from fp32 shards into MXFP8 rows: e4m3 bytes and one E8M0 scale byte per 32 elements.
 * Still ABI 7: allred_adamw_mx_bucket_f32, ALLRED_ADAMW_MX_GROUP_MAX, ALLRED_ADAMW_MX_RCEIL and
 * allred_plan_adamw_all_gather_shards_mxfp8 / allred_plan_adamw_shards_mxfp8_launches are additions — the
 * AdamW step with parameter groups inside the MXFP8 all-gather's launch: p' quantised where it is computed.
 * Still ABI 7: allred_mx2d_bucket_f32, ALLRED_MX2D_GROUP_MAX and allred_plan_all_gather_shards_mxfp8_2d /
 * allred_plan_all_gather_shards_mxfp8_2d_launches are additions — the MXFP8 all-gather that also writes the
 * column-wise rows (W^T with MX blocks along the rows of W), both from one read of the fp32 shard.
 * Still ABI 7: allred_launch_rec and allred_launch_trace_begin / allred_launch_trace_end are
 * additions — the ordered list of the kernels a thread launched; allred_last_launch is unchanged. */
#define ALLRED_ABI_VERSION 7

/* ---- status codes ---------------------------------------------------- */
#define ALLRED_OK 0
#define ALLRED_ERR_ARG (-1)          /* bad argument / size / alignment       */
#define ALLRED_ERR_SCHEDULE (-2)     /* grid is not a valid allreduce schedule */
#define ALLRED_ERR_HIP (-3)          /* HIP runtime failure                   */
#define ALLRED_ERR_RCCL (-4)         /* RCCL failure                          */
#define ALLRED_ERR_NOMEM (-5)
#define ALLRED_ERR_UNSUPPORTED (-6)
#define ALLRED_ERR_TRANSPORT (-7)    /* host exchange callback failed         */

/* ---- enums --------------------------------------------------------------*/
/* argv[1] "is swing version?" (allred_helper.cpp:205-208) */
#define ALLRED_RECDUB 0
#define ALLRED_SWING 1
/* the 1D schedules of the reference's prototypes (side_length ignored) */
#define ALLRED_RECDUB_1D 2  /* scratch_work/recdub_multicore_1D/recdub_multicore_1D.cpp:165-175 */
#define ALLRED_SWING_1D 3   /* scratch_work/all_red_swing_1D/all_red_swing_1D.cpp:32-36 */
/* which reference program: allred_BO_2D with arg 8 = 1 / = 0, allred_mem_2D */
#define ALLRED_BO 0
#define ALLRED_LO 1
#define ALLRED_MEM 2
/* execution form of a virtual-rank plan */
#define ALLRED_EXEC_STEPS 0  /* the reference's step program, step by step (partner exchange + add per step) */
#define ALLRED_EXEC_FUSED 1  /* one HBM pass for the whole allreduce, same arithmetic, same bits */
/* mem_2D accumulation (allred_mem_2D/kernels/compute_kernel.cpp:44-67) */
#define ALLRED_ACC_FP32 0    /* fp32 sum, rounded to bf16 once (default) */
#define ALLRED_ACC_BF16 1    /* the reference's bf16 dest register (fp32_dest_acc_en = false,
                                allred_helper.cpp:331-335): every add rounded to bf16 */

#define ALLRED_MAX_NODES 64
#define ALLRED_MAX_STEPS 6

const char* allred_status_string(int status);
int allred_abi_version(void);

/* ======================================================================
 * Schedule — replaces allred_helper.hpp:24-30 / allred_helper.cpp:122-191
 * and allred_BO_2D.cpp:4-5 / :217-270 (same arguments; the C++ reference
 * signatures are kept in include/allred_helper.hpp).
 * ==================================================================== */
int allred_highest_power_of_two(int value);                          /* allred_helper.cpp:122 */
uint32_t allred_get_step_directions(int node_x, int node_y);         /* allred_helper.cpp:136 */
int allred_get_comm_partner_swing_2d(int node, int step, int horizontal_step,
                                     int side_length, int total_nodes);   /* allred_helper.cpp:166 */
int allred_get_comm_partner_recdub_2d(int node, int recdub_step, int horizontal_step,
                                      int message_pass_depth, uint32_t* step_directions,
                                      int side_length);                   /* allred_helper.cpp:145 */
void allred_get_swing_block_comm_indexes(int node, int step, uint32_t* blocks /*[2]*/,
                                         int horizontal_step, int side_length,
                                         int total_nodes);                /* allred_BO_2D.cpp:220 */
void allred_get_recdub_block_comm_indexes(int node, int step, uint32_t* blocks /*[2]*/,
                                          int horizontal_step, int side_length, int total_nodes,
                                          int message_pass_depth,
                                          uint32_t* step_directions);     /* allred_BO_2D.cpp:242 */
/* NUM_TILES normalisation, allred_helper.cpp:224-234 */
int allred_normalize_tiles(int tiles, int total_nodes, int large_buffer);
/* 1D partners of the reference's 8-core prototypes */
int allred_get_comm_partner_swing_1d(int node, int step, int num_nodes);          /* all_red_swing_1D.cpp:32 */
int allred_get_comm_partner_recdub_1d(int node, int step, uint32_t* step_directions); /* recdub_multicore_1D.cpp:165 */

/* Whole per-rank schedule, as the per-core loop of allred_BO_2D.cpp:75-212
 * builds it into runtime args: partners (args 14+2i), send masks (22+2s+2i),
 * recv masks (22+4s+2i / compute args 6+2i), direction bits (arg 11).
 * Grids: side in {1,2,4,8}, total a power of two <= 64 (side*side for the
 * reference's square grids; (2,2), (2,4), (4,8) for 2/4/8 GPUs).  algo may
 * also be ALLRED_RECDUB_1D / ALLRED_SWING_1D (any power-of-two total; the
 * block masks then come from the same "reachable at later steps" rule).
 * Also validates the schedule (partners in range and symmetric, send ==
 * partner's recv, reduce-scatter leaves block r at rank r, every rank's
 * contributor sets disjoint at each merge) and derives tree_order[x]: the
 * leaf order of the reduction tree rank x evaluates, leaves(x, k) =
 * leaves(x, k-1) ++ leaves(partner_{k-1}(x), k-1); level k adds adjacent
 * groups of 2^k leaves.  LO gives rank x the value of tree x; BO gives block
 * b the value of tree b (reduced at its owner, then all-gathered).  For
 * RecDub all trees coincide; for Swing they differ (in bf16 rounding only). */
typedef struct {
    int32_t algo, side, total, steps;
    int32_t partner[ALLRED_MAX_NODES][ALLRED_MAX_STEPS];
    uint64_t send[ALLRED_MAX_NODES][ALLRED_MAX_STEPS];
    uint64_t recv[ALLRED_MAX_NODES][ALLRED_MAX_STEPS];
    uint32_t dirs[ALLRED_MAX_NODES];
    uint8_t tree_order[ALLRED_MAX_NODES][ALLRED_MAX_NODES];
} allred_schedule;
int allred_schedule_build(int algo, int side_length, int total_nodes, allred_schedule* out);
/* The fused LO pass's DAG of distinct sums (64 ranks; no reference
 * counterpart — the per-core butterfly of allred_BO_2D/kernels/
 * dataflow_kernel.cpp:19-29 evaluated once per distinct value).  Writes the
 * layout k_butterfly_lds64_pipe reads (kernels.hip) into out[cap]; returns
 * the bytes written, 0 when the schedule has no DAG form (not 64 ranks, a
 * step with more than 32 distinct sums), or a negative status.
 * *read_conflicts = extra LDS bank cycles of its reads per column group and
 * tile (0 once placed; allred_tune_set("lo_dag_place", 0) keeps first-appearance order). */
int allred_lo_dag(int algo, int side_length, int total_nodes, uint8_t* out, size_t cap, int* read_conflicts);
/* The schedule form's step program as k_steps_reg reads it (kernels.hip):
 * the per-core RS / AG loops of allred_BO_2D/kernels/dataflow_kernel.cpp:152-267
 * (variant ALLRED_BO: total x 256 bytes, one block per 256) or the LO exchange
 * steps of allred_LOO_2D/kernels/dataflow_kernel.cpp:127-175 (ALLRED_LO:
 * 2 (total/2) S + total bytes), restated on a strip's pair rows (BO: the
 * kernel recasts step 0 per block for its register-staged loads).  Returns the
 * bytes written into out[cap], 0 when the schedule has no such program, or a
 * negative status.  For inspection and CPU checks (tests/test_steps_program.py).
 * variant ALLRED_BO | ALLRED_STEPS_REG: the program k_steps_reg actually loads
 * for BO (engine.cpp bo_steps_reg_table): per block 256 bytes with step 0 recast
 * as byte u = row of step-0 pair u | 0x80 when its higher rank holds, then the
 * (total/2) pairs' (lower, higher) ranks — total x 256 + total bytes. */
#define ALLRED_STEPS_REG 0x100
int allred_steps_program(int algo, int variant, int side_length, int total_nodes, uint8_t* out, size_t cap);

/* ======================================================================
 * Host data — tt-metal bfloat16 helpers the reference calls
 * (allred_helper.cpp:277-285) and validate_result_vector (:18-120).
 * ==================================================================== */
/* create_random_vector_of_bfloat16(num_bytes, rand_max, seed): std::mt19937 +
 * uniform_real_distribution<float>(0, rand_max); two bf16 per uint32, low
 * half first.  round_mode 0 = truncating bfloat16(float) (default), 1 = RNE. */
void allred_random_bf16_vector(size_t num_bytes, int rand_max, int seed, int round_mode, uint32_t* out);
void allred_constant_bf16_vector(size_t num_bytes, float value, uint32_t* out);
/* validate_result_vector: expected = bf16((a+b) * (total_nodes/2)); prints the
 * reference's messages ("All values match!" ...) when verbose != 0.
 * Returns the number of elements with |actual - expected| > error.          */
long allred_validate_result_vector(const uint32_t* result_vec, const uint32_t* src_vec_0,
                                   const uint32_t* src_vec_1, size_t num_els, float error,
                                   uint32_t total_nodes, int verbose, float* max_error);

/* ======================================================================
 * Device compute (HIP, gfx950)
 * ==================================================================== */
/* dst[i] = bf16_rne(float(dst[i]) + float(src[i])), i < n.  Replaces the
 * per-tile add_tiles + pack_tile<true> of allred_BO_2D/kernels/compute_kernel.cpp:53-60. */
int allred_bf16_add(uint16_t* dst, const uint16_t* src, size_t n, void* stream);
/* Same over the blocks named by a 64-bit mask (block b = [b*block_elems, (b+1)*block_elems)),
 * the BO compute loop of compute_kernel.cpp:35-67 for one step. */
int allred_bf16_add_masked(uint16_t* dst, const uint16_t* src, uint64_t block_mask,
                           size_t block_elems, void* stream);

/* Reduce `total` virtual ranks (rank r at ranks + r*rank_stride) into `out`
 * with the reduction tree of rank 0 of the (algo, side, total) schedule (one
 * HBM pass; the hierarchical first stage), and the matching broadcast of one
 * vector back to every rank (the all-gather's data movement). n % 8 == 0. */
int allred_tree_reduce(const uint16_t* ranks, uint64_t rank_stride, size_t n, int algo, int side_length,
                       int total_nodes, uint16_t* out, void* stream);
int allred_broadcast(uint16_t* ranks, uint64_t rank_stride, size_t n, int total_nodes, const uint16_t* src,
                     void* stream);

/* validate_result_vector (allred_helper.cpp:18-120) on the GPU, for `rows` device-resident
 * rows at once (row r at ranks + r * rank_stride elements; pinned host rows through their
 * device pointer work too): one launch of k_validate, which reads every row once and src0 /
 * src1 once.  Per element expected = bf16((a + b) * mult) — the add, then the multiply, in
 * fp32; the conversion truncates (round_mode 0) or rounds to nearest even (1) — diff =
 * |actual - expected| in fp32, and the element is bad when !(diff <= error): NaN is bad, and so
 * is inf - inf, exactly as on the host.  mult is the reference's (float)(total_nodes / 2), or
 * any other closed form of the caller's.  Per row: bad = what allred_validate_result_vector
 * returns for it; first_bad = the lowest bad element index (UINT64_MAX: none); max_error = the
 * largest non-NaN diff over the bad elements (0: none).  The host function leaves the FIRST
 * mismatch out of its maximum (a quirk of the reference's loop, allred_helper.cpp:49-75);
 * this one does not, so the two maxima may differ by that one element.
 * Enqueues on `stream` (counters zeroed by a stream-ordered memset, the launch, the copy of the
 * `rows` records to out[], host memory) and returns once the records are on the host: it
 * synchronizes `stream` by design and must not be called while the stream is being captured
 * into a graph.  Every other call of this header that takes a plan and a stream only enqueues
 * kernel launches and can be captured.
 * ALLRED_ERR_ARG before any HIP call: a null pointer, n == 0 or n % 8 != 0, rows < 1 or
 * rows > ALLRED_MAX_NODES, rank_stride < n or % 8 != 0, a pointer not 16-byte aligned.
 * Nothing past element n of a row is read (the stride skew holds no data). */
typedef struct {
    uint64_t bad;
    uint64_t first_bad;
    float max_error;
    int32_t reserved;
} allred_rank_check;
int allred_validate_device(const uint16_t* ranks, uint64_t rank_stride, size_t n, int rows, const uint16_t* src0,
                           const uint16_t* src1, float mult, float error, int round_mode,
                           allred_rank_check* out /*[rows], host*/, void* stream);

/* ======================================================================
 * Virtual-rank plan: `total` ranks resident in ONE GPU's HBM, rank r at
 * ranks + r * rank_stride (elements).  Replaces the 64-core Tensix program
 * (allred_BO_2D/kernels, allred_LOO_2D/kernels, allred_mem_2D/kernels).
 * Every rank ends with the allreduced vector, in place.
 * ==================================================================== */
typedef struct allred_plan allred_plan;
typedef struct {
    int32_t algo;          /* ALLRED_SWING / ALLRED_RECDUB                      */
    int32_t variant;       /* ALLRED_BO / ALLRED_LO / ALLRED_MEM                */
    int32_t exec;          /* ALLRED_EXEC_STEPS / ALLRED_EXEC_FUSED             */
    int32_t side_length;   /* 1, 2, 4, 8                                        */
    int32_t total_nodes;   /* 0 = side*side                                     */
    int32_t device;        /* HIP device ordinal (-1 = current)                 */
    uint64_t elems_per_rank; /* bf16 elements; BO/MEM need a multiple of 8*total, LO of 8 */
    int32_t mem_accum;     /* MEM only: ALLRED_ACC_FP32 (default) / ALLRED_ACC_BF16 */
} allred_plan_desc;
int allred_plan_create(const allred_plan_desc* desc, allred_plan** out);
/* HBM layout helper: the rank stride (elements) this engine lays virtual ranks
 * out with — elems rounded up to 64, plus a 128-byte skew so the P rank rows
 * of a tile do not start on the same HBM channel (655,360-byte rows are
 * 5 * 2^17 apart: +5.6 % on the fused pass). */
uint64_t allred_preferred_rank_stride(uint64_t elems_per_rank);
int allred_plan_destroy(allred_plan* plan);
size_t allred_plan_workspace_bytes(const allred_plan* plan);
/* workspace: device memory of allred_plan_workspace_bytes() (may be NULL when 0) */
int allred_plan_execute(allred_plan* plan, uint16_t* ranks, uint64_t rank_stride,
                        void* workspace, void* stream);
/* The two halves of the BO allreduce as collectives of their own (sharded training:
 * (P + 1) n bytes of HBM traffic each, where the allreduce moves 2 P n).  Both take a plan
 * whose variant is ALLRED_BO (any BO grid, 2D or 1D algo; LO / MEM plans:
 * ALLRED_ERR_UNSUPPORTED); workspace may be NULL (BO plans have none).  blk =
 * elems_per_rank / total.  The argument checks are allred_plan_execute's (stride < n, stride
 * % 8, ranks not 16-byte aligned: ALLRED_ERR_ARG), made before anything is launched.  A plan
 * with total == 1 is a no-op (out of place: a copy of the one block).
 *
 * allred_plan_reduce_scatter — the RS loop of allred_BO_2D/kernels/dataflow_kernel.cpp:152-213
 * (+ compute_kernel.cpp:35-67).  In place (out == NULL): block b of rank b's row receives the
 * value the BO allreduce gives block b: tree b of the schedule (tree_order[b]), every add
 * rounded to bf16 — the bits allred_plan_execute leaves there.
 *   ALLRED_EXEC_FUSED plan: one HBM pass — the one-row tree pass with a per-block destination,
 *     k_tree / k_tree_lds / k_tree_lds_pipe with WRITE_ALL = false — that writes nothing else:
 *     every other element of every row, and everything past element n of a row, keeps its bits.
 *   ALLRED_EXEC_STEPS plan: the reference's reduce-scatter loop alone, one launch per step
 *     k = 0 .. S-1 (whatever the tune key steps_form says).  The blocks a rank does not own
 *     are left holding the reference's partial sums: UNSPECIFIED.  Nothing past element n of
 *     a row is touched.
 * Out of place (out != NULL, fused plans only; a steps-form plan: ALLRED_ERR_UNSUPPORTED):
 * rank b's reduced block goes to out + b * out_stride (blk elements) and `ranks` is only read.
 * ALLRED_ERR_ARG: out_stride < blk, out_stride % 8 != 0, out not 16-byte aligned, or
 * [out, out + total * out_stride) overlapping [ranks, ranks + total * rank_stride).
 *
 * allred_plan_all_gather — the AG loop of allred_BO_2D/kernels/dataflow_kernel.cpp:219-267.
 * In place (in == NULL): block b of rank b is copied — all 16 bits, NaN payloads included — to
 * block b of every rank (fused: one pass, k_ag; steps form: one launch per step k = S-1 .. 0).
 * Out of place (fused plans only): rank b's block is read from in + b * in_stride instead and
 * written to every rank, b included; `in` is only read; the alignment, stride and overlap
 * rules are those of `out`.  Nothing but the n elements of each row is written.
 * reduce_scatter then all_gather on one bucket = allred_plan_execute, bit for bit, in any
 * mix of fused and steps-form plans of the same schedule. */
int allred_plan_reduce_scatter(allred_plan* plan, uint16_t* ranks, uint64_t rank_stride, uint16_t* out,
                               uint64_t out_stride, void* workspace, void* stream);
int allred_plan_all_gather(allred_plan* plan, uint16_t* ranks, uint64_t rank_stride, const uint16_t* in,
                           uint64_t in_stride, void* workspace, void* stream);
/* number of kernel launches one execute enqueues (for per-launch accounting) */
int allred_plan_launches(const allred_plan* plan);

/* GROUPED calls: a list of buckets of different sizes — a training step's gradient buckets —
 * through the fused BO allreduce or its reduce-scatter in place, the small ones sharing kernel
 * launches (a fused pass below about 1024 tiles at 64 ranks is launch-bound: sixteen 32 kB
 * buckets cost sixteen launch latencies one by one).  The plan supplies the SCHEDULE only — algo,
 * side, total, the tree order table —; each bucket brings its own size, the plan's
 * elems_per_rank is not used.  Accepted plans: ALLRED_BO with ALLRED_EXEC_FUSED, any BO grid, 2D
 * or 1D algo; LO / MEM plans and steps-form plans: ALLRED_ERR_UNSUPPORTED.  No reference
 * counterpart (the reference runs one vector per program).
 *   execute_group         every bucket ends with exactly the bits allred_plan_execute of a fused
 *                         BO plan of that bucket's size gives it (block b = tree b, every add
 *                         rounded to bf16).
 *   reduce_scatter_group  block b of rank b's row of every bucket receives those bits and nothing
 *                         else is written (the other blocks, the stride skew, memory past a row),
 *                         as allred_plan_reduce_scatter in place.  Out of place: not in this call
 *                         (allred_plan_reduce_scatter_shards below).
 * Checks, all made before the first launch (a refused call writes nothing), ALLRED_ERR_ARG:
 * count < 0; buckets == NULL with count > 0; per bucket allred_plan_execute's rules (ranks NULL
 * or not 16-byte aligned, elems_per_rank == 0 or % (8 * total) != 0, rank_stride <
 * elems_per_rank or % 8 != 0); the 256-element tiles of all buckets together past 2^31 - 1
 * (32-bit tile indices); the ranges [ranks, ranks + total * rank_stride) of two buckets
 * overlapping.  count == 0: ALLRED_OK, nothing launched.  total == 1: a no-op.
 * Routing, per bucket, on the host.  A bucket keeps its own route — its own launch(es), enqueued
 * at its place in the list — when that route is the persistent 64-rank pass (64 ranks, whole
 * tiles, >= 1024 tiles, fused_form 0: HBM-bound, not launch-bound) or when it is not whole tiles
 * (total < 8 or elems_per_rank % (256 * total) != 0).  Every other bucket is whole tiles of 8 ..
 * 64 ranks: these are gathered, at most ALLRED_GROUP_MAX at a time, into ONE launch of
 * k_tree_group, enqueued when its last member is reached (the ALLRED_GROUP_MAX-th, or the end of
 * the list).  All launches go to `stream`; the buckets are disjoint, so their order among each
 * other does not matter.  The tune key pipe_grid caps the grouped grid like every persistent
 * pass; fused_form 1 or 2 turns grouping off (every bucket its own launch).  The memory type of a
 * bucket is not looked at (pinned host buckets work, without allred_plan_execute's narrow grid).
 * The grouped launch's table travels in the kernel arguments: no allocation, no copy, so the
 * calls can be captured into a graph.
 *   group_launches        the kernel launches execute_group would enqueue for the list with the
 *                         tune keys as they are now (reduce_scatter_group: the same, except that
 *                         a bucket on the persistent 64-rank route is always one launch), or a
 *                         negative status for arguments the call would refuse. */
#define ALLRED_GROUP_MAX 64            /* buckets one grouped launch covers */
typedef struct {
    uint16_t* ranks;                   /* rank r of this bucket at ranks + r * rank_stride */
    uint64_t  rank_stride;             /* elements */
    uint64_t  elems_per_rank;          /* this bucket's n; the plan's own elems_per_rank is not used */
} allred_bucket;
int allred_plan_execute_group(allred_plan* plan, const allred_bucket* buckets, int count, void* stream);
int allred_plan_reduce_scatter_group(allred_plan* plan, const allred_bucket* buckets, int count, void* stream);
int allred_plan_group_launches(const allred_plan* plan, const allred_bucket* buckets, int count);

/* GROUPED calls WITH SHARD BUFFERS: the two halves of a sharded (ZeRO / FSDP) training step over
 * the step's whole list of buckets — reduce-scatter every gradient bucket into each rank's shard,
 * (the optimizer runs on the shards,) all-gather every parameter bucket from the shards — two
 * launches per step where the per-bucket calls cost one each.  The plans, the checks and the
 * routing are the grouped calls' above: ALLRED_BO with ALLRED_EXEC_FUSED, any BO grid, 2D or 1D
 * algo (LO / MEM plans and steps-form plans: ALLRED_ERR_UNSUPPORTED); the plan supplies the
 * SCHEDULE only.  Per bucket blk = elems_per_rank / total, and shard == NULL means in place.
 * No reference counterpart (the reference runs one vector per program).
 *   reduce_scatter_shards  block b of every bucket receives the bits allred_plan_execute of a
 *                          fused plan of that size gives block b (tree b, every add rounded to
 *                          bf16).  In place it goes to rank b's own row and nothing else is
 *                          written: exactly allred_plan_reduce_scatter_group.  With a shard it
 *                          goes to shard + b * shard_stride and `ranks` is only read; every byte
 *                          outside the P blocks of blk elements keeps its bits, the gaps of a
 *                          shard_stride > blk included.
 *   all_gather_shards      block b of rank b — or of the shard — is copied, all 16 bits, NaN
 *                          payloads included, to block b of every rank.  From a shard rank b is
 *                          written too and the shard is only read; in place the owner's row is
 *                          not rewritten.  Only the n elements of each row are written.
 * Buckets with and without a shard may be mixed in one list.  reduce_scatter_shards then
 * all_gather_shards on the same list = allred_plan_execute_group, bit for bit, in place and
 * through shards.
 * Checks, all made before the first launch (a refused call writes nothing), ALLRED_ERR_ARG: those
 * of the grouped calls above for count, buckets and every bucket's ranks / rank_stride /
 * elems_per_rank, the 2^31 - 1 tile cap over the whole list included; with a shard, shard_stride
 * < blk, shard_stride % 8 != 0, a shard not 16-byte aligned, address arithmetic that would
 * overflow; an `op` other than the two constants.  count == 0: ALLRED_OK, nothing launched.
 * total == 1: a bucket in place is a no-op, one with a shard is copied by its per-bucket route.
 * DISJOINTNESS, one rule for both calls (csrc/shard_ranges.hpp): the byte sets of one list must
 * be pairwise disjoint, else ALLRED_ERR_ARG.  Every bucket's set is ONE interval, [ranks, ranks +
 * total * rank_stride) — the grouped calls' rule, the stride skew counts.  Every shard's set is
 * its `total` SEPARATE block intervals [shard + b * shard_stride, + blk); the range enclosing
 * them is not used.  Block-exact on purpose: a sharded optimizer's buffer is rank-major — one row
 * of F elements per rank, bucket i's shard at flat + off_i with shard_stride = F —, so the
 * enclosing ranges of different buckets interleave and are accepted, as are another bucket's
 * blocks in the gaps of a wide shard_stride.  Two buckets naming one shard are refused, in the
 * all-gather, which only reads it, as well.
 * Routing, per bucket, on the host, is the grouped calls' rule unchanged: a bucket keeps its own
 * launch, at its place in the list, when it is not whole tiles (total < 8 or elems_per_rank %
 * (256 * total) != 0) or when it has 64 ranks and >= 1024 tiles with fused_form 0; it then goes
 * through the per-bucket route of allred_plan_reduce_scatter(.., out, out_stride) /
 * allred_plan_all_gather(.., in, in_stride).  fused_form 1 / 2 turn grouping off.  Every other
 * bucket shares one launch per ALLRED_GROUP_MAX members: k_tree_group (no member with a shard),
 * k_tree_group with the shard table, or k_ag_group — the shard pointers travel in a second by-value table, so
 * these calls, too, can be captured into a graph.  No new tune keys: pipe_grid caps the grids
 * like every persistent pass.  The 1024-tile threshold was measured for the tree passes; nobody
 * has measured it for the all-gather, which INHERITS it so that the two halves of a step route
 * alike (one point next to it: DESIGN.md §12).
 *   shards_launches        the kernel launches the call for `op` would enqueue for the list with
 *                          the tune keys as they are now, or a negative status for arguments the
 *                          call would refuse. */
typedef struct {
    uint16_t* ranks;                   /* as allred_bucket */
    uint64_t  rank_stride;
    uint64_t  elems_per_rank;
    uint16_t* shard;                   /* NULL: in place.  Else block b of this bucket lives at
                                          shard + b * shard_stride, blk = elems_per_rank / total elements */
    uint64_t  shard_stride;            /* elements; ignored when shard == NULL */
} allred_shard_bucket;
#define ALLRED_OP_REDUCE_SCATTER 0
#define ALLRED_OP_ALL_GATHER 1
int allred_plan_reduce_scatter_shards(allred_plan* plan, const allred_shard_bucket* buckets, int count, void* stream);
int allred_plan_all_gather_shards(allred_plan* plan, const allred_shard_bucket* buckets, int count, void* stream);
int allred_plan_shards_launches(const allred_plan* plan, const allred_shard_bucket* buckets, int count, int op);

/* GROUPED calls on FP32 SHARDS: the same two halves of a sharded step for an optimizer that keeps
 * fp32 gradient shards and fp32 master parameters — the bf16 calls above would need a cast / scale
 * / accumulate pass behind the reduce-scatter and a cast pass in front of the all-gather, and their
 * tree has by then rounded every add to bf16.  Two launches per step, as above.  The accepted plans
 * are the same (ALLRED_BO with ALLRED_EXEC_FUSED, any BO grid, 2D or 1D algo; anything else:
 * ALLRED_ERR_UNSUPPORTED); the plan supplies the SCHEDULE only.  blk = elems_per_rank / total.
 * No reference counterpart, and NOT the reference's arithmetic (which stays the default everywhere
 * else): nothing here is rounded to bf16 before the shard.
 *   reduce_scatter_shards_f32  element e of block b of a bucket: s = the sum over the P ranks in
 *                          the shape of tree b (leaves in tree_order[b] order, level k adds
 *                          adjacent groups of 2^k leaves), every leaf widened bf16 -> fp32 exactly,
 *                          every add ONE IEEE fp32 add; v = s * scale, one fp32 multiply (also for
 *                          scale == 1.0f, where it is exact); shard[b * shard_stride + e] = v, or,
 *                          with ALLRED_SHARD_ACCUMULATE, = old + v as one fp32 add (never an fma).
 *                          The rank rows are only read; every byte outside the P blocks of blk
 *                          floats keeps its bits, the gaps of a wide shard_stride included; without
 *                          the flag the shard is never read.  A non-finite scale is the caller's
 *                          arithmetic and is allowed.
 *   all_gather_shards_f32  block b of EVERY rank row, rank b's included, receives
 *                          bf16_rne(shard[b * shard_stride + e]): IEEE round to nearest even, +-Inf
 *                          kept, values above the largest finite bf16 become Inf, a NaN stays a NaN,
 *                          signed zeros and denormals are not flushed.  The shard is only read and
 *                          only the n elements of each row are written.
 * Checks, all before any HIP call (a refused call writes nothing).  ALLRED_ERR_ARG: those of the
 * grouped shard calls above for the plan, count, buckets and every bucket's ranks / rank_stride /
 * elems_per_rank, the 2^31 - 1 tile cap included; per bucket shard == NULL (the shard is REQUIRED:
 * there is no in-place form), shard_stride < blk, shard_stride % 4 != 0, a shard not 16-byte
 * aligned, address arithmetic that would overflow; flags with a bit other than
 * ALLRED_SHARD_ACCUMULATE; an `op` other than the two constants.  ALLRED_ERR_UNSUPPORTED, for the
 * WHOLE list: a bucket that is not whole tiles (total < 8 or elems_per_rank % (256 * total) != 0)
 * — there is ONE kernel form for fp32 shards and no per-bucket route behind it; a flat optimizer
 * buffer is padded anyway.  count == 0: ALLRED_OK, nothing launched.
 * DISJOINTNESS is the rule above with 4-byte shard elements (csrc/shard_f32_ranges.hpp): a
 * bucket's rank rows are one interval [ranks, ranks + total * rank_stride) of 2-byte elements, its
 * shard is `total` separate block intervals of blk floats; all pairwise disjoint, else
 * ALLRED_ERR_ARG — overlapping fp32 blocks, one shard named twice and a shard on a rank row alike.
 * Routing: EVERY bucket goes through the grouped kernel, at most ALLRED_GROUP_MAX per launch —
 * k_tree_group_f32 / k_ag_group_f32 (csrc/shard_f32_kernels.hip); the tables travel by value, so
 * the calls can be captured into a graph.  shards_f32_launches is therefore ceil(count / 64) for
 * either op.  A 64-rank bucket of >= 1024 tiles stays in the grouped kernel as well: there is no
 * fp32 form of k_tree_lds_lag, and nobody has measured where one would pay — the bf16 calls'
 * 1024-tile threshold is NOT inherited here.  fused_form does not apply; pipe_grid caps the grids
 * like every persistent pass; no new tune keys. */
typedef struct {
    uint16_t* ranks;                   /* as allred_bucket: bf16 rank rows */
    uint64_t  rank_stride;             /* bf16 elements */
    uint64_t  elems_per_rank;
    float*    shard;                   /* REQUIRED: block b of this bucket at shard + b * shard_stride */
    uint64_t  shard_stride;            /* fp32 elements; >= blk, % 4 == 0 */
} allred_shard_bucket_f32;
#define ALLRED_SHARD_ACCUMULATE 1      /* flags bit 0: shard += value instead of shard = value */
int allred_plan_reduce_scatter_shards_f32(allred_plan* plan, const allred_shard_bucket_f32* buckets, int count,
                                          float scale, int flags, void* stream);
int allred_plan_all_gather_shards_f32(allred_plan* plan, const allred_shard_bucket_f32* buckets, int count, void* stream);
int allred_plan_shards_f32_launches(const allred_plan* plan, const allred_shard_bucket_f32* buckets, int count, int op);

/* The fp32 grouped reduce-scatter WITH THE GRADIENT NORM, in the same launches: what an optimizer
 * step computes between the reduce-scatter and the all-gather (clipping, the non-finite check)
 * without reading the shards back.  The SHARDS receive, bit for bit, what
 * allred_plan_reduce_scatter_shards_f32 gives them for the same arguments; accepted plans, routing,
 * launches (ceil(count / 64): allred_plan_shards_f32_launches(.., ALLRED_OP_REDUCE_SCATTER)
 * describes this call too) and graph capturability are unchanged; the rank rows are only read.
 * The kernels trace as k_tree_group_f32_norm<P, false|true>.
 *   norm_sq[b], b < total   the sum of the squares of every value this call STORED into block b of
 *                          every bucket of the list — with ALLRED_SHARD_ACCUMULATE the accumulated
 *                          old + v — in a fixed order of fp32 operations (never an fma):
 *     tile partial   a tile is 256 consecutive floats of a block: the 256 squares, one fp32 multiply
 *                    each, added as a balanced binary tree in element order (level k adds adjacent
 *                    groups of 2^k).
 *     per launch     (up to 64 consecutive buckets of the list) S = rank b's tile partials in list
 *                    order, bucket ascending, tile ascending inside block b;  a_l, l = 0 .. 63, = the
 *                    left-to-right sum of S[l], S[l + 64], S[l + 128], .. from +0.0f;  R = the balanced
 *                    binary tree over a_0 .. a_63 in index order (squares are never -0: the padding
 *                    zeros are exact no-ops).
 *     across launches  norm_sq[b] = (..(R_0 + R_1) + R_2 ..): launch 0 OVERWRITES — the old contents
 *                    of norm_sq are never read — and launch k > 0 adds its R to what launch k - 1 left.
 *   A NaN or +-Inf stored anywhere in rank b's blocks makes norm_sq[b] non-finite (compare by
 *   class): that is the found-inf signal, there is no separate counter; the other ranks' entries
 *   stay exact.  Only the `total` floats of norm_sq are written.
 * WORKSPACE: allred_plan_shards_f32_norm_workspace_bytes returns 64 + 4 T, T = the 256-element
 * tiles of the whole list counted per rank row (what the 2^31 - 1 cap counts); 0 for arguments the
 * call would refuse, 64 for count == 0.  The first 64 bytes are the arrival counter: the caller
 * ZEROES them once after allocation, every launch leaves them zero again (a captured graph replays
 * without a memset node).  The rest holds one float per tile, each launch its own region; its
 * contents afterwards are unspecified.  Nothing past the returned size is touched.  ONE WORKSPACE
 * MUST NOT BE IN FLIGHT ON TWO STREAMS at once (nor in two concurrent graph branches): calls that
 * share a workspace are ordered by the caller.
 * Checks, all before any HIP call (a refused call writes nothing): the f32 call's, unchanged, then
 * ALLRED_ERR_ARG for norm_sq NULL or not 4-byte aligned, norm_ws NULL or not 16-byte aligned, and
 * [norm_sq, + 4 total) or [norm_ws, + workspace bytes) sharing a byte with each other, with a
 * bucket's rank-row interval or with a shard block — byte-exact, the rule of
 * csrc/shard_f32_ranges.hpp, so either may lie in the gap of a wide shard_stride.  count == 0:
 * ALLRED_OK (after the pointer checks), nothing is launched and norm_sq is NOT written. */
size_t allred_plan_shards_f32_norm_workspace_bytes(const allred_plan* plan, const allred_shard_bucket_f32* buckets, int count);
int allred_plan_reduce_scatter_shards_f32_norm(allred_plan* plan, const allred_shard_bucket_f32* buckets, int count,
                                               float scale, int flags, float* norm_sq /* [total], device */,
                                               void* norm_ws /* device */, void* stream);

/* ADAMW ON THE FP32 SHARDS, INSIDE THE GROUPED ALL-GATHER'S LAUNCH: what runs between
 * allred_plan_reduce_scatter_shards_f32_norm and allred_plan_all_gather_shards_f32 — gradient
 * clipping by the global norm, the non-finite check, torch's non-amsgrad AdamW — at the point where
 * the all-gather holds every master parameter in a register anyway.  A sharded step is then TWO
 * launches: the reduce-scatter with the norm, and this call; both can be captured into one graph.
 * Accepted plans, the rank rows and blk = elems_per_rank / total are those of the fp32 calls above.
 * The kernel traces as k_adamw_ag_group_f32<P, false|true> (csrc/adamw_kernels.hip; the bool: the
 * flag below).  No reference counterpart.
 * HYPERPARAMETERS come through a DEVICE pointer (32 bytes, 16-byte aligned, only read): lr and the
 * two bias corrections change every step, and by-value arguments would be frozen into a captured
 * graph — the caller rewrites the 32 bytes with any stream-ordered copy between replays.
 * SEMANTICS.  Every operation below is ONE IEEE fp32 operation in the order written, never an fma;
 * division and square root are correctly rounded; denormals are kept.
 * Uniform values, the same for every element and every launch of the call (P = total):
 *   N    the balanced binary tree, in index order, over 64 values x_l (level k adds adjacent groups
 *        of 2^k): x_l = norm_sq[l] for l < P, +0.0f for l >= P.  norm_sq == NULL: N = +0.0f,
 *        c = 1.0f and skip is false.
 *   skip = N is NaN or +-Inf: the found-inf signal of allred_plan_reduce_scatter_shards_f32_norm.
 *   q = max_norm / (sqrtf(N) + 1e-6f);   c = (q < 1.0f) ? q : 1.0f   (max_norm = +Inf: no clipping)
 *   d = 1.0f - lr * weight_decay;   o1 = 1.0f - beta1;   o2 = 1.0f - beta2;   ss = lr / bias_corr1
 * Per element e of block b of a bucket (p, g, m, v: param, grad, exp_avg, exp_avg_sq at
 * plane[b * shard_stride + e]), when skip is false:
 *   g1  = g * c                              (also for c == 1.0f, where it is exact)
 *   p1  = p * d
 *   m'  = m * beta1 + g1 * o1
 *   v'  = v * beta2 + (g1 * g1) * o2
 *   den = sqrtf(v') / bias_corr2_sqrt + eps
 *   p'  = p1 - ss * (m' / den)
 * — torch.optim.AdamW (amsgrad = False) with m * beta1 + g * o1 written out in place of lerp.
 * STORED: p', m' and v' to their planes; block b of EVERY rank row, rank b's included, receives
 * bf16_rne(p') by all_gather_shards_f32's rounding rules.  skip: param, exp_avg and exp_avg_sq keep
 * their bits (they are not written) and the rows receive bf16_rne(p).  With ALLRED_ADAMW_ZERO_GRAD
 * every gradient element of the list is set to +0.0f, skipped step or not; without it grad is only
 * read.  hyper and norm_sq are only read.  info, when given, receives {N, c, skip ? 1.0f : 0.0f,
 * +0.0f}, written once, by the call's first launch.  Everything else keeps its bits: every byte
 * outside the P blocks of blk floats of each plane, the gaps of a wide stride, the stride skew of
 * the rows, memory past a row.
 * CHECKS, all before any HIP call (a refused call writes nothing): the plan, count, buckets, rank-row
 * rules and the 2^31 - 1 tile cap are those of the fp32 calls; a list with a bucket that is not whole
 * tiles is ALLRED_ERR_UNSUPPORTED for the whole list.  ALLRED_ERR_ARG: a NULL plane pointer, a plane
 * not 16-byte aligned, shard_stride < blk, shard_stride % 4 != 0, address arithmetic that would
 * overflow, an unknown flag bit, hyper NULL or not 16-byte aligned, norm_sq not 4-byte aligned, info
 * not 16-byte aligned.  count == 0: ALLRED_OK after the pointer checks, nothing is launched and info
 * is NOT written.
 * DISJOINTNESS (csrc/adamw_ranges.hpp; byte-exact and block-exact, else ALLRED_ERR_ARG): every
 * bucket's rank-row interval, the 4 P count plane blocks of blk floats, [hyper, + 32),
 * [norm_sq, + 4 P) and [info, + 16) are pairwise disjoint — param == grad, one plane named twice and
 * info on a row are refused alike; hyper, norm_sq and info may lie in the gap of a wide stride.
 * Four rank-major FLAT buffers, one per plane — F floats per rank, bucket i at column off_i,
 * shard_stride = F — are accepted.
 * LAUNCHES: a per-bucket entry is four pointers and a stride, so ONE launch covers
 * ALLRED_ADAMW_GROUP_MAX = 32 buckets (the kernel arguments stay below 4 KiB):
 * allred_plan_adamw_shards_f32_launches returns ceil(count / 32), or a negative status for
 * arguments the call would refuse.  pipe_grid caps the grid like every persistent pass; no new
 * tune keys. */
#define ALLRED_ADAMW_GROUP_MAX 32      /* buckets one launch of this call covers */
#define ALLRED_ADAMW_ZERO_GRAD 1       /* flags bit 0: store +0.0f over every gradient element read */
typedef struct {                       /* 64 bytes */
    uint16_t* ranks;                   /* as allred_shard_bucket_f32: bf16 rank rows, WRITTEN */
    uint64_t  rank_stride;
    uint64_t  elems_per_rank;
    float*    param;                   /* fp32 master parameters, block b at param + b * shard_stride */
    float*    grad;                    /* fp32 gradient shard: what reduce_scatter_shards_f32 filled */
    float*    exp_avg;
    float*    exp_avg_sq;
    uint64_t  shard_stride;            /* floats; ONE stride for the four planes; >= blk, % 4 == 0 */
} allred_adamw_bucket_f32;
typedef struct {                       /* 32 bytes, lives in DEVICE memory, 16-byte aligned */
    float lr, beta1, beta2, eps, weight_decay;
    float bias_corr1;                  /* 1 - beta1^t          */
    float bias_corr2_sqrt;             /* sqrt(1 - beta2^t)    */
    float max_norm;                    /* +Inf: no clipping    */
} allred_adamw_hyper;
int allred_plan_adamw_all_gather_shards_f32(allred_plan* plan, const allred_adamw_bucket_f32* buckets, int count,
                                            const allred_adamw_hyper* hyper /* device */,
                                            const float* norm_sq /* [total], device, or NULL */,
                                            float* info /* [4], device, or NULL */, int flags, void* stream);
/* Also the launch count of allred_plan_adamw_all_gather_shards_f32_groups below: its launches are the
 * same ceil(count / 32), in list order, whatever the groups are. */
int allred_plan_adamw_shards_f32_launches(const allred_plan* plan, const allred_adamw_bucket_f32* buckets, int count);

/* ADAMW PARAMETER GROUPS, STILL ONE LAUNCH PER 32 BUCKETS: allred_plan_adamw_all_gather_shards_f32
 * with a hyperparameter set per PARAMETER GROUP (torch.optim.AdamW's param_groups: biases and norm
 * weights with weight_decay = 0, layers with an lr of their own) instead of one set per call.
 * hyper is a DEVICE array of ngroups sets of 32 bytes (1 <= ngroups <= ALLRED_ADAMW_PARAM_GROUPS_MAX,
 * 16-byte aligned, only read, rewritten by the caller between graph replays like the one set);
 * group_of is a HOST array of count bytes, read during the call only: bucket i uses
 * hyper[group_of[i]].  group_of == NULL: every bucket is in group 0.  The kernel traces as
 * k_adamw_ag_groups_f32<P, false|true> (csrc/adamw_kernels.hip), ALSO for ngroups == 1: the
 * call has one kernel form, no routing rule and no tune key.  No reference counterpart.
 * SEMANTICS: those of allred_plan_adamw_all_gather_shards_f32 above, with two changes.
 *   CALL-WIDE: N, skip and c are ONE value for the whole call — gradient clipping is by the global
 *   norm over all groups, as torch.nn.utils.clip_grad_norm_ over all parameters does —, by the
 *   formulas above, with max_norm = hyper[0].max_norm.  The max_norm field of hyper[1 .. ngroups - 1]
 *   is NEVER USED.  info, when given, receives {N, c, skip ? 1.0f : 0.0f, +0.0f}, written once, by
 *   the call's first launch.
 *   PER GROUP: d, o1, o2, ss, beta1, beta2, eps and bias_corr2_sqrt are group g's, from hyper[g] by
 *   the same single fp32 operations as above (d = 1.0f - lr * weight_decay; o1 = 1.0f - beta1;
 *   o2 = 1.0f - beta2; ss = lr / bias_corr1); every element of bucket i takes group group_of[i]'s.
 * Everything else is the call's above, word for word: the per-element operations and their order (one
 * IEEE fp32 operation each, never an fma, division and square root correctly rounded, denormals
 * kept), what is STORED, the skipped step (param, exp_avg and exp_avg_sq keep their bits, the rows
 * receive bf16_rne(p)), ALLRED_ADAMW_ZERO_GRAD, and what keeps its bits.
 * GUARANTEE (tests/test_gpu_adamw_groups.py): for every bucket i the four planes and the rank rows
 * are bit for bit what allred_plan_adamw_all_gather_shards_f32 gives that bucket with the set
 * hyper[group_of[i]] whose max_norm is replaced by hyper[0].max_norm, and the same norm_sq.
 * CHECKS, all before any HIP call (a refused call writes nothing): every check of the call above,
 * unchanged, plus ALLRED_ERR_ARG for ngroups < 1 or > ALLRED_ADAMW_PARAM_GROUPS_MAX and for a
 * group_of[i] >= ngroups.  count == 0: ALLRED_OK after the pointer and ngroups checks, nothing is
 * launched and info is NOT written.
 * DISJOINTNESS: the rule above with the WHOLE array [hyper, + 32 ngroups) in place of [hyper, + 32):
 * it shares no byte with a rank-row interval, a plane block, norm_sq or info — info inside
 * hyper[ngroups - 1] is refused —, and may lie in the gap of a wide shard_stride.
 * LAUNCHES: ALLRED_ADAMW_GROUP_MAX = 32 buckets each, in list order, whatever the groups are — the
 * buckets of a group need not be adjacent; allred_plan_adamw_shards_f32_launches answers for this
 * call too.  The per-launch group table (one byte per bucket) travels by value: 3408 bytes of kernel
 * arguments. */
#define ALLRED_ADAMW_PARAM_GROUPS_MAX 8   /* hyperparameter sets one call takes */
int allred_plan_adamw_all_gather_shards_f32_groups(
    allred_plan* plan, const allred_adamw_bucket_f32* buckets,
    const uint8_t* group_of /* [count], HOST; NULL: every bucket in group 0 */, int count,
    const allred_adamw_hyper* hyper /* DEVICE, [ngroups] x 32 bytes, 16-byte aligned, only read */, int ngroups,
    const float* norm_sq /* [total], device, or NULL */, float* info /* [4], device, or NULL */,
    int flags, void* stream);

/* MXFP8 ALL-GATHER FROM THE FP32 SHARDS: allred_plan_all_gather_shards_f32 for a step that takes its
 * weights as OCP MX operands (the block-scaled f8f6f4 MFMA of the MI355X): every rank row receives the
 * shard's values as e4m3fn BYTES, and a parallel SCALE ROW receives one E8M0 byte per 32 elements.
 * The value is rounded once, from the fp32 master, in the launch that gathers it: no bf16 intermediate
 * and no quantisation pass over every rank's copy; 1.03125 bytes written per element instead of 2.
 * Accepted plans and blk = elems_per_rank / total are those of the fp32 shard calls above; the plan
 * supplies P only.  blk is a multiple of 256, so a 32-element MX block never straddles a shard block.
 * The kernel traces as k_ag_group_mxfp8<P, false|true> (csrc/mx_kernels.hip; the bool:
 * ALLRED_MX_SCALE_RCEIL).  No reference counterpart.
 * SEMANTICS.  Every output bit is a function of the input bits.  Take each aligned group of 32
 * consecutive floats x_0 .. x_31 of block b of a bucket (elements e .. e + 31 of the block, e % 32 == 0).
 * Block b of EVERY rank row, rank b's included, receives the same 32 element bytes, at byte
 * b * blk + e + i of the row; byte (b * blk + e) / 32 of EVERY scale row receives the same scale byte.
 *   A = the largest bits(x_i) & 0x7fffffff, compared as integers.
 *   A >= 0x7f800000 (a NaN or +-Inf in the block): scale byte 0xFF and all 32 element bytes 0x7F — an
 *     MX block with a NaN scale is all NaN.  This is the found-inf signal on the consumer's side.
 *   Otherwise:
 *     E = (A >> 23) - 127                      (-127 for zero and for denormals)
 *     X = E - 8                                (the floor rule of OCP MX v1.0), or, with
 *         ALLRED_MX_SCALE_RCEIL, X = E - 8 + ((A & 0x7fffff) > 0x600000 ? 1 : 0): ceil(log2(amax / 448)),
 *         under which no finite element saturates;
 *     X is clamped below at -127 (the upper clamp cannot bind: X <= 120);   scale byte = X + 127.
 *   y_i = x_i * 2^(-X): ONE fp32 multiply, denormals kept (2^(-X) is a normal fp32 for every reachable X).
 *   element byte = y_i rounded to e4m3fn: IEEE round to nearest even, subnormals as multiples of 2^-9;
 *     |y_i| > 448 gives +-448 (0x7E / 0xFE), never the NaN encoding; the sign is always kept: -0 and a
 *     negative value that rounds to zero both give 0x80.
 * The shard is only read.  Per row only elems_per_rank bytes of `rows` and elems_per_rank / 32 bytes of
 * `scales` are written; every other byte keeps its bits — stride skew, gaps, guards.
 * Dequantised value = e4m3(byte) * 2^(scale - 127).  The scale rows are PLAIN LINEAR: byte k of a scale
 * row belongs to elements 32 k .. 32 k + 31 of the element row.  The swizzled scale layouts particular
 * MFMA kernels want are the consumer's business.
 * WHAT THE MI355X MAKES OF THE ROWS (tests/test_gpu_mx_consumer.py; tests/mx_consumer.hip is the consumer).
 * The linear rows feed v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 on both sides) as they lie, with no byte
 * repacked and no scale swizzled, under this lane map, established on exact integer data: lane l of a
 * wave, g = l >> 4, loads of matrix row l & 15 the 16 bytes k0 + 16 g .. + 15 into dwords 0 .. 3 and the 16
 * bytes k0 + 64 + 16 g .. + 15 into dwords 4 .. 7, and as its scale the byte at k0 / 32 + g of the row's
 * linear scale row, which the instruction applies to bytes k0 + 32 g .. + 31.  So a lane's eight dwords are
 * NOT one MX block: they are halves of two.  The hardware's reading of every element byte under scale
 * bytes 0, 1, 8, 119, 127, 135, 246 and 254 is e4m3(byte) * 2^(scale - 127) as stated here — bias 127,
 * subnormals, signs —; 0x7F, 0xFF and a 0xFF scale (over zeros too) make all sixteen outputs of their
 * matrix row NaN and touch no other row.  A dequantised value in the fp32 denormal range is KEPT, not
 * flushed; one that overflows fp32 (256 * 2^120 under RCEIL) comes out as +-Inf of its sign.  One
 * instruction's sum over four differently scaled groups differed from the float64 product by up to
 * 9.53e-6 = 2^-16.7 times sum |a_k b_k|: more than the 2^-17 that 128 fp32 adds allow, so the matrix core
 * does not add as fp32 adds would.  The semantics above stood as written.
 * CHECKS, all before any HIP call (a refused call writes nothing).  The plan, count, sizes, overflow
 * and the 2^31 - 1 tile cap follow the fp32 shard calls.  ALLRED_ERR_ARG: a NULL rows, scales or shard;
 * rows or shard not 16-byte aligned, scales not 8-byte aligned; elems_per_rank == 0 or not a multiple
 * of 8 total; row_stride < elems_per_rank or % 16 != 0; scale_stride < elems_per_rank / 32 or % 8 != 0;
 * shard_stride < blk or % 4 != 0; address arithmetic that would overflow; a flag bit other than
 * ALLRED_MX_SCALE_RCEIL.  ALLRED_ERR_UNSUPPORTED, for the WHOLE list: a bucket that is not whole tiles
 * (total < 8 or elems_per_rank % (256 * total) != 0).  count == 0: ALLRED_OK, nothing launched.
 * DISJOINTNESS (csrc/mx_ranges.hpp; byte-exact and block-exact, else ALLRED_ERR_ARG): per bucket the
 * element rows are ONE interval [rows, rows + total * row_stride), the scale rows ONE interval
 * [scales, scales + total * scale_stride), the shard `total` separate block intervals of blk floats;
 * all pairwise disjoint, within a bucket and across buckets.  Rows or scales may sit in the gap of a
 * wide shard_stride.
 * LAUNCHES: a per-bucket table entry carries two more words than the fp32 call's, so ONE launch covers
 * ALLRED_MX_GROUP_MAX = 32 buckets (3088 bytes of kernel arguments, below 4 KiB), in list order:
 * allred_plan_all_gather_shards_mxfp8_launches returns ceil(count / 32), or a negative status for
 * arguments the call would refuse.  The tables travel by value, so the call can be captured into a
 * graph.  One kernel form, no routing rule and no tune key; pipe_grid caps the grid like every
 * persistent pass. */
#define ALLRED_MX_GROUP_MAX 32          /* buckets one launch covers */
#define ALLRED_MX_SCALE_RCEIL 1         /* flags bit 0; without it: the OCP floor rule */
typedef struct {                        /* 56 bytes */
    uint8_t*  rows;                     /* e4m3fn bytes, rank r's row at rows + r * row_stride, WRITTEN */
    uint64_t  row_stride;               /* bytes; >= elems_per_rank, % 16 == 0 */
    uint8_t*  scales;                   /* E8M0 bytes, rank r's at scales + r * scale_stride, WRITTEN */
    uint64_t  scale_stride;             /* bytes; >= elems_per_rank / 32, % 8 == 0 */
    uint64_t  elems_per_rank;
    const float* shard;                 /* as allred_shard_bucket_f32: block b at shard + b * shard_stride */
    uint64_t  shard_stride;             /* floats; >= blk, % 4 == 0 */
} allred_mx_bucket_f32;
int allred_plan_all_gather_shards_mxfp8(allred_plan* plan, const allred_mx_bucket_f32* buckets, int count, int flags,
                                        void* stream);
int allred_plan_all_gather_shards_mxfp8_launches(const allred_plan* plan, const allred_mx_bucket_f32* buckets, int count);
/* BOTH MXFP8 ORIENTATIONS FROM ONE PASS: allred_plan_all_gather_shards_mxfp8 for a weight that is used in
 * two GEMMs.  An MX block runs along the contraction dimension: Y = X W^T contracts over `in`, the columns
 * of W[out][in], and takes the rows above; the input-gradient GEMM dX = dY W contracts over `out` and
 * takes W quantised in blocks of 32 consecutive ROWS at a fixed column.  The row-wise bytes cannot serve
 * it (their scales belong to other groups of 32 elements), so a second copy must be rounded from the
 * fp32 master.  This call writes it in the launch that gathers the first, as W^T in the same plain
 * linear MX row format: what is said above of the rows and v_mfma_scale_f32_16x16x128_f8f6f4 holds for
 * the t rows as they lie, for the matrix W^T.  The AdamW step inside this launch is NOT built.
 * Accepted plans are those of allred_plan_all_gather_shards_mxfp8; the plan supplies P only.  The kernel
 * traces as k_ag_group_mxfp8_2d<P, false|true, false|true> (csrc/mx2d_kernels.hip; the bools:
 * ALLRED_MX_SCALE_RCEIL, a bucket of the launch has rows).  No reference counterpart.
 * SEMANTICS.  Every output bit is a function of the input bits.  A bucket is ONE row-major fp32 matrix
 * W[nrows][cols], nrows = elems_per_rank / cols: float i * cols + j of the bucket is W[i][j].  The
 * bucket is partitioned into `total` blocks of blk = elems_per_rank / total floats exactly as the other
 * shard calls partition it — block b at shard + b * shard_stride —, so R = nrows / total rows form a block.
 *   ROW-WISE, when rows != NULL: rows and scales receive exactly what allred_plan_all_gather_shards_mxfp8
 *   writes for the same shard and flag.
 *   COLUMN-WISE, always: for every column j and every aligned group of 32 rows 32 g .. 32 g + 31 take
 *   x_k = W[32 g + k][j] and apply to x_0 .. x_31 the rule stated above for 32 consecutive floats — the
 *   integer amax A, the NaN / Inf block, the floor or RCEIL exponent, ONE fp32 multiply, saturating RNE to
 *   e4m3fn.  The 32 element bytes go to bytes j * nrows + 32 g + k of EVERY rank's t row, the scale byte to
 *   byte j * (nrows / 32) + g of EVERY rank's t scale row.
 * A t row is therefore the linear MX row of W^T[cols][nrows]: byte k of a t scale row belongs to bytes
 * 32 k .. 32 k + 31 of the t element row.  Per rank only elems_per_rank bytes of t_rows (and of rows) and
 * elems_per_rank / 32 bytes of t_scales (and of scales) are written; every other byte keeps its bits.  The
 * shard is only read.
 * CHECKS, all before any HIP call (a refused call writes nothing).  The rules of
 * allred_plan_all_gather_shards_mxfp8 apply to rows / scales when they are given, and the same alignment
 * and stride rules to t_rows / t_scales (16 / 8 bytes; strides >= the written extent, % 16 / % 8).
 * ALLRED_ERR_ARG: exactly one of rows and scales NULL; t_rows, t_scales or shard NULL; cols == 0;
 * elems_per_rank % cols != 0; address arithmetic that would overflow; a flag bit other than
 * ALLRED_MX_SCALE_RCEIL; more than 2^31 - 1 squares of 1024 elements in the list (the launch's work
 * items are patches of whole squares).  ALLRED_ERR_UNSUPPORTED, for the WHOLE list, the MX necessities
 * only: total < 8, cols % 32 != 0, nrows % (32 * total) != 0 — a column block of 32 rows never straddles a
 * shard block and a row block never straddles a row.  count == 0: ALLRED_OK, nothing launched.
 * DISJOINTNESS (csrc/mx2d_ranges.hpp; byte-exact and block-exact, else ALLRED_ERR_ARG): per bucket up to
 * four output intervals — [rows, + total * row_stride), [scales, + total * scale_stride),
 * [t_rows, + total * t_row_stride), [t_scales, + total * t_scale_stride) — and the `total` shard block
 * intervals of blk floats; all pairwise disjoint, within a bucket and across buckets.  Outputs may sit
 * in the gap of a wide shard_stride.
 * LAUNCHES: ONE launch covers ALLRED_MX2D_GROUP_MAX = 21 buckets (96 bytes of table per bucket: 4080
 * bytes of kernel arguments, below 4 KiB), in list order: allred_plan_all_gather_shards_mxfp8_2d_launches
 * returns ceil(count / 21), or a negative status for arguments the call would refuse.  The tables travel
 * by value, so the call can be captured into a graph.  One kernel form, no routing rule and no tune key;
 * pipe_grid caps the grid like every persistent pass. */
#define ALLRED_MX2D_GROUP_MAX 21        /* buckets one launch covers */
typedef struct {                        /* 96 bytes */
    uint8_t*  rows;                     /* as allred_mx_bucket_f32; rows and scales may BOTH be NULL: column-wise only */
    uint64_t  row_stride;
    uint8_t*  scales;
    uint64_t  scale_stride;
    uint8_t*  t_rows;                   /* e4m3fn bytes of W^T, rank r's at t_rows + r * t_row_stride, WRITTEN */
    uint64_t  t_row_stride;             /* bytes; >= elems_per_rank, % 16 == 0 */
    uint8_t*  t_scales;                 /* E8M0 bytes of W^T, rank r's at t_scales + r * t_scale_stride, WRITTEN */
    uint64_t  t_scale_stride;           /* bytes; >= elems_per_rank / 32, % 8 == 0 */
    uint64_t  elems_per_rank;           /* nrows * cols */
    uint64_t  cols;                     /* the matrix's inner dimension */
    const float* shard;                 /* as allred_mx_bucket_f32 */
    uint64_t  shard_stride;
} allred_mx2d_bucket_f32;
int allred_plan_all_gather_shards_mxfp8_2d(allred_plan* plan, const allred_mx2d_bucket_f32* buckets, int count, int flags,
                                           void* stream);
int allred_plan_all_gather_shards_mxfp8_2d_launches(const allred_plan* plan, const allred_mx2d_bucket_f32* buckets, int count);
/* ADAMW INSIDE THE MXFP8 ALL-GATHER: allred_plan_adamw_all_gather_shards_f32_groups with the rows of
 * allred_plan_all_gather_shards_mxfp8 — the MXFP8 training step in TWO launches
 * (allred_plan_reduce_scatter_shards_f32_norm, then this call), as the bf16 step is.  p' is quantised
 * in the register it is computed in: no bf16 rows that nobody reads, no second pass over the masters.
 * ONE entry point and ONE kernel form, always with parameter groups: ngroups = 1 with group_of = NULL
 * is the one-set call.  hyper, group_of, ngroups, norm_sq and info are those of the groups call above;
 * rows, row_stride, scales and scale_stride those of allred_mx_bucket_f32; the four planes and
 * shard_stride those of allred_adamw_bucket_f32.  The kernel traces as
 * k_adamw_ag_mxfp8<P, false|true, false|true> (csrc/adamw_mx_kernels.hip; the bools: ALLRED_ADAMW_ZERO_GRAD,
 * ALLRED_ADAMW_MX_RCEIL).  No routing rule and no tune key; pipe_grid caps the grid like every
 * persistent pass.  No reference counterpart.
 * SEMANTICS: the two blocks above composed.
 *   NOT SKIPPED (N finite or norm_sq NULL): param, exp_avg and exp_avg_sq receive exactly the p', m'
 *   and v' that allred_plan_adamw_all_gather_shards_f32_groups stores — info, N, c and skip are the
 *   call's, max_norm is hyper[0].max_norm, d, o1, o2, ss, beta1, beta2, eps and bias_corr2_sqrt are
 *   group group_of[i]'s, every operation is ONE IEEE fp32 operation in the stated order, never an fma,
 *   division and square root correctly rounded, denormals kept — and with ALLRED_ADAMW_ZERO_GRAD +0.0f
 *   is stored over every gradient element read.
 *   Block b of EVERY rank's element row and scale row receives exactly what
 *   allred_plan_all_gather_shards_mxfp8 writes from a shard that holds p': per aligned 32 elements
 *   A = the integer maximum of bits(p'_i) & 0x7fffffff; the scale byte by the floor rule, or with
 *   ALLRED_ADAMW_MX_RCEIL by the RCEIL rule; y_i = p'_i * 2^(-X), ONE fp32 multiply; y_i rounded to
 *   e4m3fn, IEEE round to nearest even, +-448 on saturation, the sign kept; scale byte 0xFF and 32
 *   element bytes 0x7F when the block holds a NaN or +-Inf.  p' is rounded ONCE, from fp32: there is
 *   no bf16 in between.
 *   SKIPPED STEP (N non-finite): param, exp_avg and exp_avg_sq keep their bits (they are not
 *   written), the element rows and scale rows receive the quantisation of p, and
 *   ALLRED_ADAMW_ZERO_GRAD still zeroes.
 *   Everything else keeps its bits: stride skew, gaps, guards, memory past a row.
 * GUARANTEE (tests/test_gpu_adamw_mx.py): for every bucket the four planes are bit for bit those of
 * allred_plan_adamw_all_gather_shards_f32_groups on the same inputs, and the element rows and scale
 * rows are bit for bit those of allred_plan_all_gather_shards_mxfp8 (same scale rule) run on the
 * param plane that call leaves.
 * CHECKS, all before any HIP call (a refused call writes nothing).  ALLRED_ERR_ARG: a flag bit other
 * than ALLRED_ADAMW_ZERO_GRAD and ALLRED_ADAMW_MX_RCEIL; hyper NULL or not 16-byte aligned, norm_sq not
 * 4-byte, info not 16-byte aligned; ngroups < 1 or > ALLRED_ADAMW_PARAM_GROUPS_MAX, a group_of[i] >=
 * ngroups; a NULL plane or one not 16-byte aligned, shard_stride < blk or % 4 != 0; a NULL rows or
 * scales, rows not 16-byte, scales not 8-byte aligned; elems_per_rank == 0 or not a multiple of
 * 8 total; row_stride < elems_per_rank or % 16 != 0; scale_stride < elems_per_rank / 32 or % 8 != 0;
 * more than 2^31 - 1 tiles of 256 elements in the list; address arithmetic that would overflow.  The
 * plan and the count as the fp32 shard calls have them.  ALLRED_ERR_UNSUPPORTED, for the WHOLE list:
 * a bucket that is not whole tiles (total < 8 or elems_per_rank % (256 * total) != 0).  count == 0:
 * ALLRED_OK after the pointer and ngroups checks, nothing is launched and info is NOT written.
 * DISJOINTNESS (csrc/adamw_mx_ranges.hpp; byte-exact and block-exact, else ALLRED_ERR_ARG): per bucket
 * the element rows are ONE interval [rows, rows + total * row_stride), the scale rows ONE interval
 * [scales, scales + total * scale_stride), and each of the four planes `total` separate block
 * intervals of blk floats; against those stand [hyper, + 32 ngroups), [norm_sq, + 4 total) and
 * [info, + 16) where given.  All pairwise disjoint, within a bucket and across buckets.  Rows, scales
 * and the three small buffers may lie in the gap of a wide shard_stride.
 * LAUNCHES: ALLRED_ADAMW_MX_GROUP_MAX = 32 buckets each (3920 bytes of kernel arguments, below 4 KiB),
 * in list order, whatever the groups are: allred_plan_adamw_shards_mxfp8_launches returns
 * ceil(count / 32), or a negative status for arguments the call would refuse (it takes no hyper).
 * The tables travel by value, so the call can be captured into a graph; hyper is rewritten by the
 * caller between replays. */
#define ALLRED_ADAMW_MX_GROUP_MAX 32     /* buckets one launch of this call covers */
#define ALLRED_ADAMW_MX_RCEIL 2          /* flags bit 1; bit 0 stays ALLRED_ADAMW_ZERO_GRAD */
typedef struct {                        /* 80 bytes */
    uint8_t*  rows;                     /* as allred_mx_bucket_f32: e4m3fn bytes, WRITTEN */
    uint64_t  row_stride;               /* bytes; >= elems_per_rank, % 16 == 0 */
    uint8_t*  scales;                   /* as allred_mx_bucket_f32: E8M0 bytes, WRITTEN */
    uint64_t  scale_stride;             /* bytes; >= elems_per_rank / 32, % 8 == 0 */
    uint64_t  elems_per_rank;
    float*    param;                    /* as allred_adamw_bucket_f32: block b at plane + b * shard_stride */
    float*    grad;
    float*    exp_avg;
    float*    exp_avg_sq;
    uint64_t  shard_stride;             /* floats, ONE stride for the four planes; >= blk, % 4 == 0 */
} allred_adamw_mx_bucket_f32;
int allred_plan_adamw_all_gather_shards_mxfp8(
    allred_plan* plan, const allred_adamw_mx_bucket_f32* buckets,
    const uint8_t* group_of /* [count], HOST; NULL: every bucket in group 0 */, int count,
    const allred_adamw_hyper* hyper /* DEVICE, [ngroups] x 32 bytes, 16-byte aligned, only read */, int ngroups,
    const float* norm_sq /* [total], device, or NULL */, float* info /* [4], device, or NULL */,
    int flags, void* stream);
int allred_plan_adamw_shards_mxfp8_launches(const allred_plan* plan, const allred_adamw_mx_bucket_f32* buckets, int count);
/* Device-side profiling of the schedule form (the reference's DeviceZoneScopedN
 * "ALL_RED_LOOP", allred_BO_2D/kernels/dataflow_kernel.cpp:147, dumped by
 * DumpDeviceProfileResults, allred_helper.hpp:88).  stamp_words: the uint64
 * words of device memory execute_profiled writes (0: this plan's form has no
 * stamps — only ALLRED_EXEC_STEPS BO / LO do).  rank_zones: from the stamps
 * copied to the host, each rank's zone start / end (s_memrealtime, 100 MHz):
 * start = its first load, end = the end of the step of its last store. */
uint64_t allred_plan_stamp_words(const allred_plan* plan);
int allred_plan_execute_profiled(allred_plan* plan, uint16_t* ranks, uint64_t rank_stride, void* workspace,
                                 uint64_t* device_stamps, void* stream);
int allred_plan_rank_zones(const allred_plan* plan, const uint64_t* host_stamps, uint64_t* zone_start /*[total]*/,
                           uint64_t* zone_end /*[total]*/);

/* ======================================================================
 * Tuning: the one entry point for switching between kernel forms that give
 * bit-identical results (A/B measurements).  The defaults are the measured
 * product forms; nothing needs setting.  Initial values may come from
 * ALLRED_TUNE="key=value,key=value" (read once at load).  Keys:
 *   fused_form        0 auto | 1 register tree | 2 one tile per workgroup | 3 persistent pipe
 *   lo_tree           1: fused LO of rank-uniform schedules through the BO tree pass
 *   lo_dag            1: fused 64-rank LO as the DAG of distinct sums (0 = per-rank butterfly)
 *   lo_dag_place      1: bank-conflict-free DAG placement (0 = first-appearance order)
 *   lo_dag_min_tiles  256: smallest bucket (256-element tiles) for the DAG pass
 *   mem_reduce_lds    1: mem_2D schedule-form reduce staged through LDS
 *   steps_form        schedule form: 0 one pipelined launch (units staged into LDS two ahead, the step
 *                     program among LDS rows, stores one unit late) | 1 one launch per step (rank
 *                     copies in the buckets) | 2 one launch with every unit resident at once
 *   pipe_grid         0: auto grid of the persistent passes
 *   lo_dag_reg        1: fused LO of the non-rank-uniform Swing schedules (32 / 64 ranks) as the
 *                     build-time DAG of distinct sums in registers (0 = the LDS DAG pass above)
 *   lo_dag_reg_min_tiles  64: smallest bucket (256-element tiles per rank, 32 kB) for lo_dag_reg
 *   check             0; 1: check mode of the N > 1 step programs (allred_dist_allreduce and its
 *                     host twin): each rank's program is verified once against its partners'
 *                     (what a partner sends at step k is exactly what this rank receives; the
 *                     received runs of a step are disjoint, inside the bucket) — ALLRED_ERR_SCHEDULE
 *                     if not — and every receive region is filled with 0xFFFF (a bf16 NaN) before
 *                     its step, so an element the transport never delivered surfaces as NaN in the
 *                     result instead of stale data.  Same result bits on a correct run.  (The
 *                     reference has no invariant or race checking)
 *   fused_chunk_tiles 1280: the persistent fused 64-rank passes run a bucket of T 256-element
 *                     tiles as max(1, round(T / 1280)) launches over consecutive tile ranges
 *                     (0 = one launch); allred_plan_launches counts them
 *   lo_tree_min_tiles 64: a 64-rank rank-uniform LO plan (every RecDub schedule) takes the BO tree
 *                     pass from this many 256-element tiles per rank, the register butterfly below
 *   tree_bcast_lag    1: k_tree_bcast_x (allred_dist_allreduce_pipelined) stores the previous
 *                     bucket's rows of a tile one iteration after the tile's tree (0: in the same one)
 *   tree_bcast_bal    0; 1: k_tree_bcast_x spreads the result-tile loads and partial stores over
 *                     its four waves (8 columns each) instead of wave 0
 *   steps_groups      0: workgroups per CU of the schedule form k_steps_reg — 0 auto (BO 3; LO 4,
 *                     or 3 where 4 would leave every wave exactly one strip), 3, 4 or 5 (1 and 2:
 *                     ALLRED_ERR_ARG)
 *   steps_tab         1: k_steps_reg (BO) stages only the programs of its own units' blocks (when fewer
 *                     than P); 0: every block's program (P x 256 bytes) per workgroup (round 3)
 *   steps_early       1: k_steps_reg issues the first strip's loads before it stages its programs when
 *                     its grid is full (units >= workgroups), else after; 2: always before; 0: always
 *                     after (round 3)
 *   peer_fence        0; 1: the flag protocols of the peer windows (k_peer_oneshot, k_peer_sched,
 *                     k_peer_sched_push) put a system-scope release fence before every flag store
 *                     and an acquire fence after every flag wait.  Same bits; the default relies on
 *                     the ordering argument of DESIGN.md §5 (uncached hand-off memory, s_waitcnt
 *                     before the workgroup barrier that precedes a flag).  The LL kernels have no
 *                     separate flag (each word carries its epoch) and take no fence.  Every rank
 *                     must use the same setting
 *   hier_ws_ahead     1: k_hier_ws's reducing waves load one tile ahead; 2: two (measured slower,
 *                     +0.3-0.5 us at W = 1)
 *   hier_ws_cols      16: 16-byte columns of a tile per k_hier_ws reducing wave — 8 (quarters: 8
 *                     waves per workgroup), 16 (halves: 4 waves) or 32 (whole tiles: 2 waves); other
 *                     values ALLRED_ERR_ARG
 *   multi_fault       0; fault injection (tests only): 1..32: GPU value - 1 of allred_run_multi fails its
 *                     timed allreduce while its peers are in theirs (every thread must return);
 *                     33..64: GPU value - 33 fails its warm-up (every thread skips the timed region)
 *   rccl_fault        0; fault injection of the bounded RCCL waits (tests only), a bit mask: 1 init,
 *                     2 every group end, 4 every allred_comm_wait stays pending as if a peer never
 *                     arrived, so the deadline / ncclCommAbort path runs (ALLRED_ERR_TRANSPORT)
 * Plans read the keys when they are created (lo_*, steps_form) or launched.
 * ALLRED_ERR_ARG: unknown key or value out of range.  No reference
 * counterpart (the reference picks its kernel directory by string,
 * allred_BO_2D.cpp:203-211). */
int allred_tune_set(const char* key, int64_t value);
int allred_tune_get(const char* key, int64_t* value);

/* The last kernel launch of the calling thread among the ones the bench
 * reports (the fused BO pass k_tree_lds_lag, the schedule form k_steps_reg,
 * the hierarchical one-launch steps k_hier_ws / k_hier_x2): the kernel, the
 * grid its launcher chose, and — queried at this call — its static LDS,
 * VGPRs, resident workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor)
 * and the device's CU count.  ALLRED_ERR_ARG when this thread launched none of
 * them.  No reference counterpart (the reference fixes its core grid,
 * allred_BO_2D.cpp:26). */
typedef struct {
    char kernel[64];
    uint32_t grid;
    uint32_t block;
    uint32_t lds_bytes;
    int32_t regs;
    int32_t resident_per_cu;
    int32_t cus;
    int32_t device;
    int32_t reserved;
} allred_launch_info;
int allred_last_launch(allred_launch_info* out);

/* The launch trace of the calling thread: EVERY kernel the one-GPU engine (and the peer
 * kernels allred_last_launch reports) launches between begin and end, in launch order.
 * Names carry the template arguments ("k_tree_lds<16, true>", "k_mem_lds_lag<false>",
 * "k_lo_dag_reg<LoDag0>"); a call that enqueues nothing records nothing.
 * allred_launch_trace_begin arms the trace and clears it.  allred_launch_trace_end disarms
 * it, copies the first min(cap, 64, *count) records to out and sets *count to the number of
 * launches seen: the trace is a fixed ring of 64 records without allocation, launches beyond
 * 64 are counted and not stored.  Disarmed, a launch pays one thread-local load and a branch.
 * Launches made by other threads (the worker threads of allred_run_multi) are not seen.
 * ALLRED_ERR_ARG: count NULL, cap < 0, out NULL with cap > 0, or end without begin.
 * allred_last_launch neither feeds on nor is changed by the trace.  No reference counterpart. */
typedef struct {
    char kernel[64];
    uint32_t grid;     /* workgroups (x; multiplied out when the grid is 2D) */
    uint32_t block;
} allred_launch_rec;
int allred_launch_trace_begin(void);
int allred_launch_trace_end(allred_launch_rec* out, int cap, int* count);

/* ======================================================================
 * Reference program surface: AllredConfig (allred_helper.hpp:47-97) +
 * the mains of allred_BO_2D.cpp:7-215 / allred_LO_2D.cpp:9-106 /
 * allred_mem_2D.cpp:4-165, with the same 8 positional arguments.
 * ==================================================================== */
typedef struct {
    int32_t variant;         /* ALLRED_BO (bo flag decides BO vs LO), ALLRED_LO (legacy binary), ALLRED_MEM */
    int32_t swing;           /* argv[1] == 1                                     */
    int32_t run_kernel;      /* argv[2] == 1                                     */
    int32_t side_length;     /* highest_power_of_two(argv[3])                    */
    int32_t seed;            /* argv[4]: < 0 -> all ones                          */
    int32_t tiles;           /* argv[5] (raw, >= 1)                              */
    int32_t error;           /* argv[6]                                          */
    int32_t print_core;      /* argv[7]                                          */
    int32_t bandwidth_optimal; /* argv[8]                                        */
    int32_t total_nodes;     /* extension (ALLRED_NODES env / argv[9]); 0 = side^2 */
    int32_t exec;            /* extension (ALLRED_EXEC env): fused (default) / steps */
    int32_t round_mode;      /* extension (ALLRED_BF16_ROUND env): 0 trunc, 1 rne */
    int32_t num_tiles;       /* derived: normalised NUM_TILES                    */
    int32_t device;          /* HIP device ordinal, -1 = current (ALLRED_DEVICE env); the
                                reference's CreateDevice(0) / IDevice*, allred_BO_2D.cpp:8 */
    int32_t mem_accum;       /* extension (ALLRED_MEM_ACC=bf16): ALLRED_ACC_FP32 / ALLRED_ACC_BF16 */
    int32_t gpus;            /* extension (argv[10] or ALLRED_GPUS): 0 = every rank a virtual rank on
                                `device` (the default); G >= 1 = the ranks spread over GPUs
                                device .. device + G - 1, one host thread and one RCCL rank per GPU */
} allred_args;
/* Parses argv exactly like AllredConfig's ctor (std::stoi semantics: leading
 * integer, junk -> ALLRED_ERR_ARG where the reference would throw).          */
int allred_args_parse(int argc, const char* const* argv, int variant, allred_args* out);

typedef struct {
    int64_t mismatches;      /* validate_result_vector count, -1 if not run      */
    float max_error;
    double device_seconds;   /* hipEvent time of the device-resident allreduce */
    double e2e_seconds;      /* pinned H2D + allreduce + D2H                     */
    uint64_t bytes_per_rank;
    int32_t total_nodes;
    int32_t launches;
} allred_report;
/* Generate inputs, H2D, run (if run_kernel), D2H of print_core, validate
 * (printing like the reference when verbose), report timing, on args->device.
 * args->gpus = G >= 1 (ALLRED_GPUS / argv[10]): the same program on G GPUs of
 * this node in ONE process, one host thread per GPU, one RCCL communicator per
 * GPU (ncclCommInitAll).  The total_nodes ranks are split into G groups of
 * L = total / G consecutive ranks, group g on GPU device + g (G a power of two
 * dividing total, G <= the visible GPUs; else ALLRED_ERR_ARG before any HIP
 * call).  L == 1: the reference's own (side, total) schedule runs across the
 * GPUs (allred_dist_allreduce: Swing / RecDub BO or LO, or mem_2D's
 * one-shot exchange); L > 1: each GPU reduces its L ranks with the (side, L)
 * sub-grid's tree (or (2,2)/(2,4)/(4,8)/... when the rows do not form one),
 * the GPUs allreduce the partials on the (2,2)/(2,4)/(4,8) grid, and every
 * rank gets the result (mem_2D: L == 1 or G == 1 only, else
 * ALLRED_ERR_UNSUPPORTED).  Every GPU's first rank is validated as well as
 * print_core (ALLRED_CHECK_ALL: every rank); device_seconds / e2e_seconds are
 * the slowest GPU's.  The reference is single-chip (allred_BO_2D.cpp:7-29,
 * allred_helper.cpp:205-220): this is its argv across the GPUs of one node.
 * ALLRED_PROFILE_LOG=<path> also writes every rank's ALL_RED_LOOP zone in the
 * layout of tt-metal's profile_log_device.csv (the reference's
 * TT_METAL_DEVICE_PROFILER=1 run, python/timing_taker.py:60-65).            */
int allred_run(const allred_args* args, int verbose, allred_report* report);
/* allred_run with the data in the caller's hands (allred_run(a, v, r) is
 * allred_run_io(a, v, r, NULL, NULL, NULL)):
 *   in_all      NULL, or total * elems bf16 rank-major inputs of the caller's own (arbitrary
 *               data: validation is skipped, report->mismatches = -1, as allred_run_multi);
 *   out_all     NULL, or total * elems bf16 receiving every rank's result, rank-major;
 *   result_vec  NULL, or num_els = elems / 2 packed words receiving print_core's result: the
 *               reference's AllredConfig::result_vec (allred_helper.hpp:92).
 * elems = num_tiles * 1024.  With run_kernel == 0 both receive the unreduced inputs.  A failed
 * call writes neither.  args->gpus > 0 dispatches like allred_run (ALLRED_TRANSPORT /
 * ALLRED_SHARE_GPU) and forwards the buffers to allred_run_multi: with ALLRED_TRANSPORT=host
 * the whole call makes no HIP call.  On one GPU every end-to-end mode (ALLRED_E2E=zerocopy |
 * dma, ALLRED_E2E_CHUNKS) gives the bits of the plan on the same data; with in_all the
 * column-chunked DMA form runs only where a column chunk's pass is that bit for bit (schedules
 * whose per-block trees coincide: every RecDub grid, Swing up to 16 ranks), else the buckets go
 * as one copy each way.
 * ALLRED_CHECK_ALL=device (one GPU): the ranks other than print_core are counted by
 * allred_validate_device on the memory the result lives in (the device rows of the DMA modes,
 * the pinned buckets through their device pointer in zero-copy mode) instead of N - 1 host
 * passes; report->mismatches is the same number.  print_core still goes through the host
 * validator and its printed report.  The multi-GPU path ignores `device`. */
int allred_run_io(const allred_args* args, int verbose, allred_report* report, const uint16_t* in_all,
                  uint16_t* out_all, uint32_t* result_vec);

/* ======================================================================
 * Multi-GPU: one process per GPU, RCCL point-to-point over xGMI.
 * The grid (side_length, total_nodes) maps GPUs onto the reference's own
 * 2D schedule: 2 GPUs (2,2), 4 GPUs (2,4), 8 GPUs (4,8).
 * ==================================================================== */
#define ALLRED_UNIQUE_ID_BYTES 128
typedef struct allred_comm allred_comm;
int allred_comm_get_unique_id(uint8_t* id /*[128]*/);
int allred_comm_init(const uint8_t* id, int nranks, int rank, int device, allred_comm** out);
/* ndev communicators in ONE process (ncclCommInitAll), rank i on devices[i]:
 * one host thread per communicator afterwards (each thread its own stream).
 * The reference's CreateDevice(0) (allred_BO_2D.cpp:8) for the GPUs of a node. */
int allred_comm_init_all(int ndev, const int* devices, allred_comm** out /*[ndev]*/);
int allred_comm_destroy(allred_comm* comm);

typedef struct {
    int32_t algo;           /* ALLRED_SWING / ALLRED_RECDUB                     */
    int32_t variant;        /* ALLRED_BO, ALLRED_LO, or ALLRED_MEM (local_ranks == 1: the
                               mem_2D one-shot exchange, allred_mem_2D.cpp:4-165 — every
                               rank's copy of block b to rank b, summed there in mem_2D
                               order, then gathered; all links at once)      */
    int32_t side_length;    /* GPU grid                                         */
    int32_t total_nodes;    /* == nranks                                        */
    uint64_t elems;         /* bf16 elements per GPU bucket (multiple of 8*total for BO) */
    /* hierarchical extension: the bucket holds local_ranks virtual ranks
     * (stride `elems`), reduced on-GPU first with the local_side grid. 1 = flat. */
    int32_t local_ranks;
    int32_t local_side;
    int32_t local_algo;
    int32_t channels;       /* link-spreading channels: 0 = auto (all 2^S-1 links for
                               buckets >= 1 MiB on XOR grids), 1 = the plain schedule */
    int32_t mem_accum;      /* ALLRED_MEM only: ALLRED_ACC_FP32 (default) / ALLRED_ACC_BF16 */
} allred_dist_desc;
/* Scratch device bytes the call needs (recv staging + hierarchical partial). */
size_t allred_dist_workspace_bytes(const allred_dist_desc* desc);
int allred_dist_allreduce(allred_comm* comm, const allred_dist_desc* desc, uint16_t* buf,
                          void* workspace, void* stream);

/* The hierarchical step (local_ranks > 1, BO / LO) PIPELINED across consecutive
 * buckets: the call with `cur` reduces cur's local ranks to its partial (the
 * local tree), FUSED with writing the previous call's bucket's rows from its
 * allreduced partial (one HBM pass, k_tree_bcast_x, reads and writes of the two
 * buckets overlapping), then runs the RCCL program on cur's partial; cur ==
 * NULL (flush) writes the last pending bucket's rows.  K buckets = K + 1 calls:
 * b0, b1, ..., b_{K-1}, NULL.  A bucket's rows are final, in stream order,
 * after the next call (or the flush): keep it alive until then.  workspace:
 * 2 * allred_dist_workspace_bytes(desc) bytes (two parities), the same on every
 * call of a sequence; every call of a sequence has the same elems and
 * local_ranks (else ALLRED_ERR_ARG).  Same result bits as allred_dist_allreduce
 * per bucket.  The reference runs one vector per program: no counterpart. */
int allred_dist_allreduce_pipelined(allred_comm* comm, const allred_dist_desc* desc, uint16_t* cur, void* workspace,
                                    void* stream);
/* The two local phases of the pipelined step as one call: cur's tree (local
 * rank 0's, as allred_tree_reduce) into cur_out, and prev_src to every one of
 * prev's `total` rank rows (as allred_broadcast). */
int allred_tree_broadcast_pipelined(uint16_t* cur, uint16_t* prev, uint64_t rank_stride, size_t n, int algo,
                                    int side_length, int total_nodes, uint16_t* cur_out, const uint16_t* prev_src,
                                    void* stream);

/* The per-rank program allred_dist_allreduce (and its host twin) runs for
 * `desc`: steps = exchange steps (one RCCL group each), add_launches = add
 * kernels it enqueues over all steps (one per reduce-scatter / LO step,
 * whatever the channel count), segments = send + receive segments.  Programs
 * are built once per (desc, rank) and cached. */
int allred_dist_program_stats(const allred_dist_desc* desc, int rank, int* steps, int* add_launches, int* segments);

/* Host-memory twin of allred_dist_allreduce for CPU tests and loopback
 * checks: the same per-rank step program, exchanges done by a callback.     */
typedef struct {
    void* ptr;
    uint64_t bytes;
} allred_seg;
/* Exchange with `peer`: send every send segment, receive every recv segment
 * (in list order on both sides).  Return 0 on success. */
typedef int (*allred_exchange_fn)(void* ctx, int peer, int nsend, const allred_seg* send,
                                  int nrecv, const allred_seg* recv);
int allred_dist_allreduce_host(const allred_dist_desc* desc, int rank, uint16_t* buf,
                               uint16_t* scratch, allred_exchange_fn exchange, void* ctx);

/* The halves of the per-rank BO program as calls of their own: the program is S
 * reduce-scatter steps (allred_BO_2D/kernels/dataflow_kernel.cpp:152-213) followed by S
 * all-gather steps (:219-267); these run the first S, or the last S, steps of the SAME cached
 * program (same segments, adds, bounded waits; check mode verifies the steps that run and
 * poisons their receive regions).  After reduce_scatter rank r's block r (elems / total
 * elements at r * elems / total) is final — the BO allreduce's bits — and its other blocks are
 * UNSPECIFIED (the reference's partial sums); after all_gather every rank holds every owner's
 * block, copied bit for bit.  reduce_scatter then all_gather = allred_dist_allreduce with
 * channels = 1.  ALLRED_ERR_UNSUPPORTED (before any exchange): a variant other than
 * ALLRED_BO, local_ranks > 1, channels > 1 (0 and 1 both mean the plain schedule here: with
 * link-spreading channels the block a rank owns differs per channel).  workspace:
 * allred_dist_workspace_bytes(desc); scratch: elems elements. */
int allred_dist_reduce_scatter(allred_comm* comm, const allred_dist_desc* desc, uint16_t* buf, void* workspace,
                               void* stream);
int allred_dist_all_gather(allred_comm* comm, const allred_dist_desc* desc, uint16_t* buf, void* workspace,
                           void* stream);
int allred_dist_reduce_scatter_host(const allred_dist_desc* desc, int rank, uint16_t* buf, uint16_t* scratch,
                                    allred_exchange_fn exchange, void* ctx);
int allred_dist_all_gather_host(const allred_dist_desc* desc, int rank, uint16_t* buf, uint16_t* scratch,
                                allred_exchange_fn exchange, void* ctx);

/* ---- bounded RCCL (a bad configuration returns an error
 * instead of hanging; the reference hangs, allred_helper.hpp:84-96) -------
 * Communicators are created non-blocking (ncclConfig_t.blocking = 0): init
 * and every ncclGroupEnd are polled (ncclCommGetAsyncError) against a
 * deadline; allred_comm_wait polls the stream the same way.  Past the
 * deadline the communicator is aborted (ncclCommAbort: its kernels leave
 * their waits) and the call returns ALLRED_ERR_TRANSPORT; every later call
 * on that communicator returns ALLRED_ERR_TRANSPORT too (destroy it).
 * timeout_ms: 0 = the default, ALLRED_RCCL_TIMEOUT_MS or 4000 ms for
 * operations (init: at least 60 s — a node's first RCCL init takes seconds). */
int allred_comm_set_timeout(allred_comm* comm, int timeout_ms);
/* Waits until `stream` has drained (hipStreamQuery) or the deadline passed
 * (-> ncclCommAbort, ALLRED_ERR_TRANSPORT); an asynchronous RCCL error ->
 * ALLRED_ERR_RCCL.  Replaces hipStreamSynchronize after RCCL work. */
int allred_comm_wait(allred_comm* comm, void* stream);
/* 1 once the communicator was aborted, else 0. */
int allred_comm_aborted(const allred_comm* comm);

/* ======================================================================
 * allred_run across GPUs (args->gpus = G >= 1) in two parts.
 * (1) The PLAN — pure host computation, no HIP call: how the reference's
 *     (side, total) ranks (allred_BO_2D.cpp:7-29, allred_helper.cpp:205-220)
 *     split over G GPUs and which exchange every GPU runs.
 * (2) An EXCHANGE BACKEND executing it, one host thread per GPU:
 *   ALLRED_TRANSPORT_RCCL  one RCCL rank per GPU (allred_comm_init_all +
 *                          allred_dist_allreduce), the default;
 *   ALLRED_TRANSPORT_PEER  peer windows of the G threads mapped into each other
 *                          in-process (allred_peer_connect_all) and
 *                          allred_peer_dist_allreduce; with share_device every
 *                          group runs on ONE GPU (a rehearsal of the G-GPU
 *                          orchestration on hardware: threads, barriers, per-GPU
 *                          H2D / D2H slices, validation);
 *   ALLRED_TRANSPORT_HOST  the host twin: G threads on host memory running
 *                          allred_dist_allreduce_host with an in-memory exchange;
 *                          no HIP call at all (CPU tests of the orchestration;
 *                          only ever selected explicitly).
 * allred_run picks them from ALLRED_TRANSPORT=rccl|peer|host and
 * ALLRED_SHARE_GPU=1.
 * ==================================================================== */
#define ALLRED_MULTI_FLAT 0   /* L = 1: the reference's own (side, total) schedule across the GPUs */
#define ALLRED_MULTI_HIER 1   /* L > 1: each GPU's L ranks -> its sub-grid's tree, the partials
                                 allreduced on the (2,2)/(2,4)/(4,8)... GPU grid, the result written
                                 to every rank: a hierarchical COMPOSITION — on arbitrary data its
                                 bits differ from the flat one-GPU plan of the same argv; on the
                                 reference's own inputs both are exactly RNE(a+b)*N/2 */
#define ALLRED_MULTI_LOCAL 2  /* G = 1, mem_2D: the fused mem_2D pass over every rank, no exchange */
#define ALLRED_TRANSPORT_RCCL 0
#define ALLRED_TRANSPORT_PEER 1
#define ALLRED_TRANSPORT_HOST 2
typedef struct {
    int32_t gpus;             /* G                                                   */
    int32_t local_ranks;      /* L = total / G: ranks g*L .. g*L + L - 1 live on GPU g */
    int32_t total_nodes;
    int32_t variant;          /* ALLRED_BO / ALLRED_LO / ALLRED_MEM, as executed      */
    int32_t mode;             /* ALLRED_MULTI_*                                      */
    int32_t print_core;       /* validated with the reference's printed report        */
    uint64_t elems;           /* bf16 elements per rank                              */
    uint64_t validated_mask;  /* bit r: rank r goes through validate_result_vector    */
    allred_dist_desc desc;    /* the exchange every GPU runs (FLAT / HIER)            */
} allred_multi_plan;
/* check_all != 0: every rank validated (ALLRED_CHECK_ALL), else print_core and
 * every GPU's first rank.  ALLRED_ERR_ARG / _SCHEDULE / _UNSUPPORTED exactly
 * where allred_run refuses the split (before any HIP call). */
int allred_multi_plan_build(const allred_args* args, int check_all, allred_multi_plan* out);
typedef struct {
    int32_t transport;        /* ALLRED_TRANSPORT_*                                  */
    int32_t share_device;     /* 1: every group on args->device (PEER / HOST only)     */
    int32_t timeout_ms;       /* RCCL deadline (0 = default); HOST: exchange deadline */
    int32_t reserved;
} allred_multi_opts;
/* allred_run's multi-GPU form with an explicit backend.  in_all: NULL (the
 * reference's generated inputs, validated as allred_run does), or total * elems
 * bf16 rank-major inputs of the caller's own (arbitrary data: validation is
 * skipped, report->mismatches = -1).  out_all: NULL, or total * elems bf16
 * receiving every rank's result (rank-major) for checks. */
int allred_run_multi(const allred_args* args, const allred_multi_opts* opts, int verbose, allred_report* report,
                     const uint16_t* in_all, uint16_t* out_all);

/* ======================================================================
 * Peer-mapped one-shot allreduce across GPUs: the shared-memory variant
 * (allred_mem_2D.cpp:4-165) with every GPU's window IPC-mapped into every
 * peer (one process per GPU).  Result semantics = allred_mem_2D: block b is
 * owner b's copy + every other rank's copy in rank order, fp32, one rounding.
 *   create -> handle (256 bytes, exchange with every rank) -> connect(all
 *   handles in rank order) -> allreduce ... -> destroy.
 * Barriers spin with a bound; allred_peer_status() reports bit 0 = timeout,
 * and the WIN/FLAGS_CACHED bits when uncached (fine-grained) device memory
 * was unavailable and ordinary hipMalloc memory had to be used instead.
 * A timed-out call has produced wrong bytes: callers must check the status
 * (allred_peer_status after the stream, or allred_peer_check) before using
 * results; the first timeout makes every later wait of that launch give up.
 * ==================================================================== */
#define ALLRED_PEER_HANDLE_BYTES 256
/* largest IPC-exported window: a peer's hipIpcOpenMemHandle of a ~2 GiB
 * allocation never returned on the MI355X boxes (profiles/r01_peer_open_probe_2gib_hang.txt),
 * so allred_peer_create rejects max_elems * 2 > 1 GiB (ALLRED_ERR_ARG) */
#define ALLRED_PEER_MAX_WINDOW_BYTES (1ull << 30)
#define ALLRED_PEER_TIMEOUT 0x1u
#define ALLRED_PEER_WIN_CACHED 0x100u
#define ALLRED_PEER_FLAGS_CACHED 0x200u
typedef struct allred_peer allred_peer;
int allred_peer_create(int nranks, int rank, int device, uint64_t max_elems, allred_peer** out);
int allred_peer_handle(allred_peer* peer, uint8_t* handle /*[ALLRED_PEER_HANDLE_BYTES]*/);
int allred_peer_connect(allred_peer* peer, const uint8_t* all_handles /*[nranks * ALLRED_PEER_HANDLE_BYTES]*/);
/* The peers of ONE process (peers[q] = rank q, one host thread per rank
 * afterwards): every window mapped into every peer directly, no IPC (peer
 * access enabled between distinct devices).  Replaces handle + connect when
 * the ranks are threads (allred_run across GPUs, ALLRED_TRANSPORT_PEER). */
int allred_peer_connect_all(int nranks, allred_peer* const* peers);
/* elems % (8 * nranks) == 0, elems <= max_elems.  local_ranks > 1: `buf`
 * holds local_ranks virtual ranks (stride elems) reduced on-GPU first
 * (tree of local rank 0) into `workspace` (elems * 2 bytes), then broadcast. */
int allred_peer_allreduce(allred_peer* peer, uint16_t* buf, uint64_t elems, int local_ranks, int local_side,
                          int local_algo, void* workspace, void* stream);
/* The hierarchical step of allred_peer_allreduce (64 local ranks per GPU, the
 * same result bits) PIPELINED across consecutive buckets, two deep
 * (k_hier_x2): the call with cur starts it
 * (tree, partials pushed to the owners), sums the owned tiles of the bucket
 * the previous call started and writes the rank rows of the bucket started
 * two calls earlier; cur == NULL (flush) finishes every pending bucket in one
 * launch.  K buckets = K + 1 calls: b0, b1, ..., b_{K-1}, NULL.  A bucket's
 * rows are final, in stream order, after the call that started the bucket
 * two calls later (or the flush); keep it alive until then.  Every poll of a
 * launch waits for pushes of the previous launch on the other GPUs, so a GPU
 * up to one launch late stalls nobody.  While buckets are pending, the other
 * peer allreduce calls return ALLRED_ERR_ARG; so does another bucket size
 * mid-sequence or a flush with nothing pending.  ALLRED_ERR_UNSUPPORTED:
 * local_ranks != 64, more than 8 GPUs, flags not uncached, or a bucket beyond
 * the hand-off area (elems > min(max_elems, 4 Mi)).  Any grid cap
 * (allred_peer_set_max_groups) works: a workgroup runs any number of tiles, its
 * results staged in LDS 8 tiles at a time.  (The one-deep form of rounds 3-5,
 * k_hier_x, is retired: 15.1-15.3 us at W = 1 against this form's 15.0.)
 * No reference counterpart (the reference runs one vector per program). */
int allred_peer_allreduce_pipelined2(allred_peer* peer, uint16_t* cur, uint64_t elems, int local_ranks,
                                     int local_side, int local_algo, void* stream);
/* Buckets of at most `bytes` (default 4 MiB) run as one kernel (per-workgroup
 * flags, no kernel boundaries); larger ones as copy / barrier / reduce-scatter /
 * barrier / all-gather launches.  Same result bits either way.  Every rank
 * must use the same setting. */
int allred_peer_set_oneshot_max(allred_peer* peer, uint64_t bytes);
/* enable = 1 (the default): with local_ranks == 64 and nranks <= 8,
 * allred_peer_allreduce runs the hierarchical step as ONE kernel, k_hier_ws,
 * with LL hand-offs (each cross-GPU transfer a push of self-validating 8-byte
 * data+epoch words into the consumer's own memory; no flags, no remote reads)
 * and reducing and writing waves in every workgroup, so each CU reads and
 * writes at once, for buckets of up to min(max_elems, 4 Mi) elements that are
 * a multiple of 256 x nranks (others run the launch form).  0 = the launch
 * form (tree, the mem_2D exchange, broadcast as launches).  Same result bits
 * either way (allred_mem_2D semantics over the per-GPU trees); other values
 * ALLRED_ERR_ARG.  Every rank must use the same setting.  Replaces nothing in
 * the reference (its mem_2D phases sync through semaphores,
 * allred_mem_2D/kernels/dataflow_kernel.cpp:201-230).  (Retired forms and
 * their numbers at W = 1, profiles/README.md: k_hier_ll — the three phases in
 * sequence, 16.2 us vs k_hier_ws's 14.5-14.6 — in round 6; the per-tile flag
 * form, 19.9 us, and the pipelined LL form, 17.8 us, in round 5; the
 * specialised-wave form of round 1, 27-38 us.)  ABI 7: 2 is no longer a value. */
int allred_peer_set_hier_ll(allred_peer* peer, int enable);
/* Caps the grid of the hierarchical one-kernel forms, k_peer_mem_ll and the
 * scheduled form (allred_peer_dist_allreduce) at `groups` workgroups (0 =
 * default: 512 for the hierarchical forms, two per CU, 256 for the scheduled
 * form; the whole grid resident on a GPU of its own).
 * Their workgroups wait for each other across processes, so when several
 * processes share one GPU (rehearsals) the sum of their grids must fit at once:
 * groups <= 512 / processes.  Same result bits at any cap. */
int allred_peer_set_max_groups(allred_peer* peer, uint32_t groups);
/* allred_peer_dist_allreduce runs one-channel LO buckets of at most `bytes`
 * (default 256 KiB; 0 = never) with LL hand-offs (k_peer_lo_ll: each step
 * pushes data+epoch words into the partner's memory and polls its own — one
 * one-way xGMI trip per step instead of a flag and a remote read).  Same
 * result bits.  Every rank must use the same setting.  Replaces the semaphore
 * handshake + NoC write of allred_LOO_2D/kernels/dataflow_kernel.cpp:127-175. */
int allred_peer_set_lo_ll_max(allred_peer* peer, uint64_t bytes);
/* allred_peer_allreduce (mem_2D) runs buckets of at most `bytes` (default
 * 256 KiB; 0 = never) with LL hand-offs (k_peer_mem_ll: block copies pushed to
 * their owners, owners push the sums; two one-way xGMI trips, no flags, no
 * remote reads), larger ones as before.  Same result bits.  Every rank must
 * use the same setting. */
int allred_peer_set_mem_ll_max(allred_peer* peer, uint64_t bytes);
/* allred_peer_dist_allreduce runs BO buckets of at least `min_bytes` (default
 * 0 = never) in the PUSH form (k_peer_sched_push): each exchange is written by
 * the sender into the receiver's staging window (reduce-scatter) or main window
 * (all-gather) and announced with a flag, instead of read by the receiver
 * over xGMI — posted writes, no read round trips.  Same program, same adds,
 * same result bits.  Every rank must use the same setting.  Replaces the NoC
 * writes of allred_BO_2D/kernels/dataflow_kernel.cpp:152-267 (the reference's
 * sender also writes into the receiver's L1). */
int allred_peer_set_sched_push(allred_peer* peer, uint64_t min_bytes);
/* The allred_dist_allreduce program (same desc, same result bits: Swing /
 * RecDub BO or LO, link-spreading channels, hierarchical local ranks) with
 * RCCL replaced by direct reads of the partners' IPC-mapped windows: one
 * kernel, each step waits only for its partner (allred_BO_2D
 * dataflow_kernel.cpp:152-267 semaphore handshakes, over xGMI).
 * desc->variant ALLRED_MEM runs allred_peer_allreduce (fp32 accumulation only: mem_accum
 * ALLRED_ACC_BF16 -> ALLRED_ERR_UNSUPPORTED; RCCL runs it).  desc->total_nodes
 * must equal nranks; elems <= max_elems (BO) or max_elems / 2 (LO);
 * workspace: allred_dist_workspace_bytes(desc) bytes when local_ranks > 1. */
int allred_peer_dist_allreduce(allred_peer* peer, const allred_dist_desc* desc, uint16_t* buf, void* workspace,
                               void* stream);
int allred_peer_status(allred_peer* peer, uint32_t* status);
/* Synchronises `stream` and returns ALLRED_ERR_TRANSPORT if any call so far
 * timed out (ALLRED_PEER_TIMEOUT), else ALLRED_OK. */
int allred_peer_check(allred_peer* peer, void* stream);
/* Clears the status word (ALLRED_PEER_TIMEOUT is sticky: once set, every later bounded
 * wait of this peer gives up at once) through the null stream, and nothing else.  Call
 * with no kernel of this peer in flight (after allred_peer_check).  The call counter
 * keeps advancing, so the next call's LL words and flags carry epochs no timed-out call
 * wrote.  Returns ALLRED_ERR_ARG while a pipelined sequence (allred_peer_allreduce_pipelined2)
 * is pending: finish it first.  ABI 5. */
int allred_peer_clear_status(allred_peer* peer);
int allred_peer_destroy(allred_peer* peer);

#ifdef __cplusplus
}
#endif
#endif /* ALLRED_H */
