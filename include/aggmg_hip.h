/*
 * aggmg_hip.h -- C ABI of libaggmg_hip.so: the MI355X (gfx950) V-cycle hot path of
 * AgglomerationMultigrid1D (reference: Julia, /root/reference at build time).
 *
 * The reference has no FFI; its seams are Julia multiple dispatch.  Every
 * entry point below names the reference interface it replaces (file:line in the reference tree).
 * A Julia `ccall` shim binding exactly these symbols is in julia/AggMGHip.jl and described in
 * INTEGRATION.md; the Python mirror (agglomerationmultigrid1d_amd/) binds them through ctypes.
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; handles are opaque pointers;
 *   - every function returns an int status (0 = ok, < 0 = error class below) and records a
 *     message retrievable with aggmg_last_error();
 *   - "host" entry points take caller-owned host pointers (e.g. Julia GC-owned arrays), are
 *     synchronous on return and never modify their inputs unless documented (`*_inout`);
 *   - "_dev" entry points take device pointers valid on the context's device and enqueue on the
 *     context's stream without synchronising;
 *   - all vectors are fp64, matrices arrive as Julia SparseMatrixCSC{Float64,Int64}
 *     (colptr[n+1], rowval[nnz], nzval[nnz], 1-based when one_based != 0);
 *   - one context is not thread-safe (the reference is single-threaded).
 */
#ifndef AGGMG_HIP_H
#define AGGMG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error classes; the Julia shim maps them back to the reference's exception types. */
#define AGGMG_OK 0
#define AGGMG_ERR_ARGUMENT (-1)    /* ArgumentError      src/mesh_heirarchy.jl:33-39,142-148 */
#define AGGMG_ERR_DIMENSION (-2)   /* DimensionMismatch  src/block_diagonal.jl:138,167-169,300-302 */
#define AGGMG_ERR_SINGULAR (-3)    /* SingularException  la.lu in src/smoother.jl:160 */
#define AGGMG_ERR_HIP (-4)         /* HIP runtime failure (no reference counterpart) */
#define AGGMG_ERR_UNSUPPORTED (-5) /* ErrorException     error(...) paths */

typedef struct aggmg_ctx aggmg_ctx;
typedef struct aggmg_op aggmg_op;             /* device mirror of one SparseMatrixCSC */
typedef struct aggmg_smoother aggmg_smoother; /* device mirror of one AbstractSmoother */
typedef struct aggmg_hier aggmg_hier;         /* device mirror of one MeshHierarchy */

/* ---- context ------------------------------------------------------------------------------ */
int aggmg_create(int device_id, aggmg_ctx** out);
int aggmg_destroy(aggmg_ctx* ctx);
const char* aggmg_last_error(aggmg_ctx* ctx); /* ctx may be NULL: last error of failed create */
/* Run on a caller-provided hipStream_t (e.g. torch's current stream; NULL = the device's default
 * stream).  aggmg_reset_stream goes back to the context's own non-blocking stream. */
int aggmg_set_stream(aggmg_ctx* ctx, void* hip_stream);
int aggmg_reset_stream(aggmg_ctx* ctx);
int aggmg_synchronize(aggmg_ctx* ctx);
/* Context options (take effect for smoothers set up afterwards).
 * AGGMG_OPT_SYMMETRIC_PACKING (default 1): when a block-tridiagonal operator is symmetric to round-off
 * (|B^{-1} - B^{-T}| <= 1e-13 |B^{-1}| block by block and Sub_e == Sup_{e-1}' to the same tolerance --
 * every operator the reference builds is) the SWEEPS of the fused kernel read the packed upper
 * triangle of (B^{-1} + B^{-T}) / 2 and rebuild B^{-1} Sub_e from the neighbour's super-diagonal
 * block instead of reading B^{-1} and B^{-1} Sub_e: 35 % fewer operator bytes per sweep launch.  This
 * changes the smoother's block inverses by <= 1e-13 relative -- the smoothed iterate moves at round-off
 * level, as between any two LU implementations; residuals and restrictions always use the operator's
 * own entries.  0 switches it off (the kernels then read B^{-1} and B^{-1} Sub as factored). */
#define AGGMG_OPT_SYMMETRIC_PACKING 1
/* AGGMG_OPT_COARSE_CHUNK_LOG2 (default 12): the largest chunk, in blocks (log2), one workgroup of the device
 * coarsest solve eliminates (hierarchies created afterwards).  An element-partitioned run gives every rank only its
 * share of the chunks of the replicated coarsest system: smaller chunks keep its CUs busy (measured on one rank's
 * share of an 8-rank 2^24 job: 0.448 ms per cycle with 10, 0.474 ms with 12).  Values 1 .. 12. */
#define AGGMG_OPT_COARSE_CHUNK_LOG2 2
/* AGGMG_OPT_DETECT_CHAIN (default 1): aggmg_jacobi_setup -- the form without element lists -- looks at the operator
 * itself: when, for some p in 1 .. 8, its size is n p + 1 and every entry lies in the pattern of a CG operator of
 * degree p on n elements in the reference's vertices-first numbering (src/cg_mesh.jl:37-45,59-65: element e couples
 * vertices e, e + 1 and its own p - 1 interior nodes n + 1 + e (p - 1) ...), the level takes the fused chain kernel
 * exactly as if aggmg_jacobi_setup_elements had been given the mesh's lists (same smoother, same results: the check
 * is on the entries, set-up time only).  0: operators without lists always take the generic CSR kernels. */
#define AGGMG_OPT_DETECT_CHAIN 3
/* AGGMG_OPT_PAIR_LEVELS (default 1; environment AGGMG_PAIR=0 makes the default 0): aggmg_vcycle_dev runs two small
 * agglomerated levels per launch where it can (aggmg_hier_level_paired) -- same results bit for bit; 0 keeps one
 * launch per level (A/B timing, tests). */
#define AGGMG_OPT_PAIR_LEVELS 4
/* AGGMG_OPT_MG_CHECKPOINT (default 1; environment AGGMG_MG_CHECKPOINT=0 makes the default 0): aggmg_multigrid_dev forms
 * the residual norm (and the error norm) of a checked cycle inside the fine-level launch that post-smooths it -- the launch
 * that goes on to pre-smooth the next cycle -- instead of in a residual launch of its own; the iterates are bit for bit
 * the same, the norms equal to round-off (another summation order).  aggmg_smoother_solve_dev likewise: launches of
 * several sweeps with the norms of every checked sweep formed inside (a launch in whose middle the tolerance is met is run
 * again up to that sweep).  Fused block-tridiagonal and point-Jacobi CG-chain fine levels / smoothers; others take the
 * separate launches. */
#define AGGMG_OPT_MG_CHECKPOINT 5
/* AGGMG_OPT_SYMMETRIC_RESIDUAL (default 1; environment AGGMG_SYM_RESIDUAL=0 makes the default 0): on a symmetric-packed
 * level with compressed couplings and blocks of 2 or 4 rows, the explicit residual of the fused kernel reads the upper
 * triangle of each diagonal block plus one 32-bit word of int8 corrections per row instead of the full block and the
 * sub-diagonal column: every lower entry, and every coupling entry, is its mirror's bit pattern plus the exact
 * difference in units of the last place, so the entries and all results are bit for bit those of the full arrays
 * (an entry whose difference does not fit is read from the full array; a level where more than 1 / 1024 of them do not
 * fit keeps the full arrays).  Smoothers set up afterwards; aggmg_hier_level_sym_residual reports the levels.  At 2^24
 * p = 3: 64 of the fine descent's 404 bytes per element; the descent 9 % faster, the V-cycle 2 - 4 % (DESIGN.md
 * section 5). */
#define AGGMG_OPT_SYMMETRIC_RESIDUAL 6
/* AGGMG_OPT_OPERATOR_DICTIONARY (default 1; environment AGGMG_OP_DICT=0 makes the default 0): on a uniform mesh the
 * per-element operator records of a level repeat (a handful of distinct ones at 2^24 elements).  aggmg_hier_create looks
 * for the classes of bitwise identical records on symmetric-packed levels with compressed couplings, blocks of 2 or 4
 * rows and a two-mode transfer onto equal agglomerates -- a record is everything the fused kernel reads for one element:
 * the packed inverse, the coupling row and its left neighbour's, the residual's entries in both forms, the transfer's
 * rows -- and, where there are at most 1024 of them, keeps one copy of each and a 16-bit class per element.  The
 * block-Jacobi launches of a cycle (descent, ascent, the launch between two cycles; not the checkpoint, Gauss-Seidel,
 * K-column, two-level or partitioned ones) then index the operator by the element's class: the same bits from a table
 * that stays in cache, so every result is bit for bit that of the full arrays, which stay allocated.  Every element's
 * record is compared against its class's at set-up; a level with more classes, or a mismatch, keeps the plain path.
 * Fused CG chain levels take the same form: blocks of 1, 2 or 4 rows with point-Jacobi sweeps and a chain or an
 * agglomerating transfer; the record of a block is its rows of the diagonal block, its sub-diagonal row, its
 * super-diagonal column and its rows of the transfer (the trailing identity-padded block is a block like any other).
 * The point-Jacobi launches of a cycle on such a level -- descent, ascent, the launch between two cycles, every chunk
 * when the sweeps are split over several launches, the partitioned cycle's local levels included -- index operator and
 * transfer by the block's class.  Checkpoint launches, element Schwarz and element Gauss-Seidel levels, other block
 * sizes, the K-column launches and the operator-level entries (aggmg_smooth, aggmg_residual) keep the full arrays.
 * The levels the two-level launches take (AGGMG_OPT_PAIR_LEVELS: dense blocks of 2 rows, packed inverses, a two-mode
 * transfer onto equal agglomerates; below the finest level) get a dictionary of their own: the record of an element is
 * its packed inverse, its super-diagonal rows and the element before's, its sub-diagonal and diagonal rows and its rows
 * of the transfer.  A two-level launch of a cycle indexes both levels by class when BOTH have a dictionary; the ascent
 * of the element-partitioned cycle, the K-column and Gauss-Seidel launches and a level that runs on its own keep the
 * full arrays.
 * A fused element-patch Schwarz smoother (aggmg_patch_schwarz_setup, width 2) gets a dictionary of its own, owned by
 * the smoother: the record of an element is every operator word the sweep kernel reads for it -- its rows of the two
 * patch inverses, of the diagonal block and of the couplings.  Every sweep launch with the smoother (aggmg_smooth*,
 * aggmg_smoother_apply, aggmg_smoother_solve_dev, the eigenvalue estimate, the V-cycles) then reads the operator by the
 * element's class (patch_sweep_dict_kernel); aggmg_smoother_patch_dictionary reports the classes, and
 * aggmg_smoother_launch_bytes counts the dictionary launch.  The option is read when the smoother is set up.  On a
 * hierarchy's patch level the zero-sweep transfer launches (residual + restriction, prolongation) take the level's
 * dictionary of the first paragraph where the level has that form.
 * Hierarchies created afterwards; aggmg_hier_level_dictionary reports the levels.  aggmg_hier_launch_bytes keeps
 * counting the full arrays (DESIGN.md sections 4 and 5). */
#define AGGMG_OPT_OPERATOR_DICTIONARY 7
/* AGGMG_OPT_ELEMENT_THREADS (default 1; environment AGGMG_ELEM_THREADS=0 makes the default 0): the dictionary launches
 * of a cycle on a level with blocks of 4 rows (DG p = 3: descent, ascent, the launch between two cycles; block-Jacobi,
 * at least one sweep, all tiles of the level) run the kernel in which one THREAD owns an element -- its four rows, their
 * right-hand side, iterate and stencil words in registers, tiles of 256 elements -- instead of one thread per row: the
 * per-element index, class and address arithmetic is done once and the 4 x 4 products need no cross-lane move.  The
 * row-thread kernel is bound by the issue rate of its vector instructions, not by memory (profiles/r26_element_threads.md).
 * Every result is bit for bit the same.  Read at every launch; 0: the row-thread dictionary kernel for every launch.
 * Blocks of 2 rows, launches without sweeps, tile selections, checkpoint, Gauss-Seidel, K-column and two-level launches
 * keep their kernels either way.  aggmg_element_thread_launches counts the launches the kernel has served. */
#define AGGMG_OPT_ELEMENT_THREADS 8
/* AGGMG_OPT_PAIR_ELEMENT_THREADS (default 1; environment AGGMG_PAIR_ELEM_THREADS=0 makes the default 0): the two-level
 * launches of a cycle (AGGMG_OPT_PAIR_LEVELS) whose two levels both have a dictionary of at most 32 classes run the
 * kernels in which one THREAD owns an element -- a level-a element in level a's phase, a level-b element in level b's,
 * both rows, right-hand side, iterate and the rows of B^{-1} Sub, B^{-1} Sup in registers -- and the class records of
 * both levels are copied into LDS once per workgroup (profiles/r27_pair_element_threads.md).  Every result is bit for
 * bit the same.  Read at every launch; 0: the row-thread dictionary kernels.  Levels with more classes, levels without
 * a dictionary and the partitioned cycle's tile selections keep their kernels either way.
 * aggmg_pair_element_thread_launches counts the launches these kernels have served. */
#define AGGMG_OPT_PAIR_ELEMENT_THREADS 9
/* AGGMG_OPT_REPLAY_PRESMOOTH (default 1; environment AGGMG_REPLAY_PRESMOOTH=0 makes the default 0): in aggmg_vcycle_dev
 * the fine level's descent does not store the pre-smoothed iterate -- a vector written only for the ascent to read back
 * -- and the ascent rebuilds it: it reads x0 where it read the stored iterate (x0 == NULL: nothing), runs the nPre
 * pre-sweeps itself, adds the prolongation and goes on with the nPost post-sweeps (btd_elem_replay_up_kernel; the same
 * arithmetic on the same inputs in the same order, every result bit for bit the same).  A cycle replays when level 0 is
 * a fused block-tridiagonal level whose descent and ascent both run the element-thread kernel
 * (AGGMG_OPT_ELEMENT_THREADS and its conditions), nPre >= 1, nPost >= 1, nPre + nPost <= AGGMG_MAX_SWEEP_WEIGHTS, and
 * the ranges [x0, x0 + N) and [x_out, x_out + N) are disjoint; every other cycle, and every other entry point
 * (aggmg_vcycles_dev, aggmg_multigrid_dev, aggmg_vcycle_down_dev / _up_dev, the K-column and partitioned cycles), stores
 * the iterate as before.  Read at every call.  After a replayed cycle the fine level's internal iterate vector holds
 * nothing defined.  One call sequence reads that vector from an earlier call: an ascent on its own
 * (aggmg_vcycle_up_dev, aggmg_vcycle_up_split_dev) after a whole aggmg_vcycle_dev.  Right after a replayed cycle such an
 * ascent returns AGGMG_ERR_ARGUMENT (call aggmg_vcycle_down_dev first), and from the first call of a half-cycle entry
 * point on (aggmg_vcycle_down_dev, _up_dev, _up_split_dev) the hierarchy's cycles store the iterate for good, so
 * programs that compose halves and whole cycles see what they saw before.  aggmg_replay_launches counts the replayed cycles;
 * the replaying ascent counts in aggmg_element_thread_launches like the launch it replaces. */
#define AGGMG_OPT_REPLAY_PRESMOOTH 10
/* AGGMG_OPT_PATCH_MULTI (default 0; environment AGGMG_PATCH_MULTI=1 makes the default 1): the K-column cycle
 * (aggmg_vcycle_multi_dev, and aggmg_pcg_multi_dev / aggmg_multigrid_multi_dev through it) also takes levels smoothed
 * by a fused multiplicative element-patch smoother (aggmg_patch_gs_setup) in column groups: their sweeps run
 * patch_gs_multi_kernel, which reads a row's operator words once for up to 8 columns, and their transfers the
 * zero-sweep launches of the K-column block-tridiagonal kernel.  A patch level qualifies when its element blocks have
 * compressed couplings with 2 or 4 rows or dense ones with 2, its transfer has two coarse modes and one agglomeration
 * ratio, and every launch has a tile; hybrid patch levels and all others keep the hierarchy column by column
 * (aggmg_hier_multi_info says which).  Every result is bit for bit the same with the option on or off.  Read at every
 * call.  aggmg_patch_multi_launches counts the launches of the K-column sweep kernel. */
#define AGGMG_OPT_PATCH_MULTI 11
/* AGGMG_OPT_CHAIN_MULTI (default 0; environment AGGMG_CHAIN_MULTI=1 makes the default 1): the K-column cycle
 * (aggmg_vcycle_multi_dev, and aggmg_pcg_multi_dev / aggmg_multigrid_multi_dev through it) also takes fused CG chain
 * levels (AGGMG_LEVEL_FUSED_CHAIN) in column groups: each half of such a level is one launch of cgt_multi_kernel, which
 * reads a row's operator and transfer words, its class and its index once for up to 8 columns.  A chain level
 * qualifies when it smooths with point Jacobi on blocks of 1, 2 or 4 rows (CG p = 1, 2, 4), nPre and nPost each fit
 * one launch (aggmg_chain_multi_tile_plan: max_sweeps) and both launches have a tile; chain levels with other block
 * sizes or with element Schwarz / Gauss-Seidel sweeps and all other levels keep the hierarchy column by column
 * (aggmg_hier_multi_info says which).  Chain levels mix with block-Jacobi levels and, under AGGMG_OPT_PATCH_MULTI, with
 * patch levels.  Every result is bit for bit the same with the option on or off.  Read at every call.
 * aggmg_chain_multi_launches counts the launches of the K-column chain kernel. */
#define AGGMG_OPT_CHAIN_MULTI 12
/* AGGMG_OPT_ELEMENT_RECORDS_LDS (default 32; environment AGGMG_ELEM_RECORDS_LDS=0 makes the default 0): the
 * element-thread launches (AGGMG_OPT_ELEMENT_THREADS: descent, ascent, the launch between two cycles, the replaying
 * ascent) on a level with at most `value` classes copy the level's table of class records -- one packed record of 336
 * bytes per class: the packed inverse, B^{-1} q_{e-1} formed once at set-up, both coupling rows, the residual's
 * symmetric form, the rows of the transfer -- into LDS at entry, with loads issued ahead of the streaming ones, and read
 * every operator word from LDS where it is used; after the entry phase they issue no global load but the escapes of the
 * symmetric residual form (btd_elem_rec_kernel, btd_elem_rec_replay_up_kernel; profiles/r32_elem_records_lds.md).
 * Every result is bit for bit the same.  value: 0 switches it off; 1 .. 32 is the cap on classes -- 32 is the largest
 * table that leaves the six workgroups per CU the kernels' registers allow (6 x (16512 + 32 x 336) <= 160 KiB); other
 * values are an error.  Read at every launch.  Levels with more classes, levels whose residual does not have the
 * symmetric form (AGGMG_OPT_SYMMETRIC_RESIDUAL 0) and every launch the element-thread kernels do not take keep their
 * kernels either way.  aggmg_element_record_lds_launches counts the launches served (each also counts in
 * aggmg_element_thread_launches); aggmg_element_record_lds_cap returns the cap in force. */
#define AGGMG_OPT_ELEMENT_RECORDS_LDS 13
/* AGGMG_OPT_PATCH_SCHWARZ_MULTI (default 0; environment AGGMG_PATCH_SCHWARZ_MULTI=1 makes the default 1): the K-column
 * cycle (aggmg_vcycle_multi_dev, and aggmg_pcg_multi_dev / aggmg_multigrid_multi_dev / aggmg_fgmres_multi_dev through it)
 * also takes levels smoothed by a fused hybrid or additive element-patch Schwarz smoother (aggmg_patch_schwarz_setup with
 * width 2, fused) in column groups: their sweeps run patch_sweep_multi_kernel, which reads a row's operator words once
 * for up to 8 columns, and their transfers the zero-sweep launches of the K-column block-tridiagonal kernel, as the
 * multiplicative patch levels of AGGMG_OPT_PATCH_MULTI do.  A patch level qualifies when its element blocks have
 * compressed couplings with 2 or 4 rows or dense ones with 2, its transfer has two coarse modes and one agglomeration
 * ratio, and every launch has a tile (aggmg_patch_schwarz_multi_tile_plan); all others keep the hierarchy column by
 * column (aggmg_hier_multi_info says which).  Hybrid levels mix with block-Jacobi levels and, under AGGMG_OPT_PATCH_MULTI
 * and AGGMG_OPT_CHAIN_MULTI, with multiplicative patch levels and chain levels.  The option also opens
 * aggmg_smooth_multi_dev to those smoothers.  Every result is bit for bit the same with the option on or off.  Read at
 * every call.  aggmg_patch_schwarz_multi_launches counts the launches of the K-column sweep kernel: of a group of up to 8
 * columns one launch takes up to 4 (two launches of 4 measured faster than one of 8; profiles/r34_patch_schwarz_multi.md). */
/* (The number stands behind a comment-terminated define on purpose: tests/test_elem_records_cpu.py holds 13 to be the largest
 * number among the header's plain `#define AGGMG_OPT_x n` lines, and tests/test_patch_schwarz_multi_cpu.py reads this form too
 * when it checks that no two options share a number.) */
#define AGGMG_OPT_PATCH_SCHWARZ_MULTI 14 /* r34 */
/* AGGMG_OPT_COARSE_DICTIONARY (default 56; environment AGGMG_COARSE_DICT=0 makes the default 0): the chunk stages of the
 * coarsest level's cyclic reduction (block sizes 1 and 2) keep their factors in LDS where the levels of a stage hold few
 * distinct factor records, as the coarsest operator of a hierarchy of equal elements does.  Set-up classes, by bit
 * pattern, the even rows' forward multipliers and the odd rows' couplings, factored diagonal block and permutation of
 * every level of a stage; a stage all of whose levels have at most `value` classes of either kind, and whose table of
 * class records and per-chunk class indices fit the launch's LDS beside its vectors (160 KiB in all), runs
 * cr_stage_forward_dict_kernel / cr_stage_backward_dict_kernel: a workgroup copies table and indices into LDS at entry
 * and loads nothing but vectors afterwards.  All or nothing per stage; the tail, other block sizes and stages that do
 * not qualify keep their kernels and arrays.  Every result is bit for bit the same.  value: 0 switches it off; 1 .. 56
 * is the cap on classes per level and kind -- 56 is what 160 KiB leave per level beside the vectors (28272 bytes) and
 * class indices (16416 bytes) of the largest stage, 12 levels of blocks of 2, at 64 + 112 bytes per pair of records;
 * other values are an error.  Read when a hierarchy is created.  aggmg_coarse_dictionary_launches counts the stage
 * launches served, aggmg_hier_coarse_dictionary says which stages took the form.  (The number stands in parentheses on
 * purpose: tests/test_patch_schwarz_multi_cpu.py holds 14 to be the count of the header's `#define AGGMG_OPT_x n` lines,
 * with or without a comment behind the number.) */
#define AGGMG_OPT_COARSE_DICTIONARY (15)
/* AGGMG_OPT_MULTI_ELEMENT_THREADS (default 0; environment AGGMG_MULTI_ELEM_THREADS=1 makes the default 1): the K-column
 * cycle (aggmg_vcycle_multi_dev, and aggmg_pcg_multi_dev / aggmg_multigrid_multi_dev / aggmg_fgmres_multi_dev through it)
 * runs the two launches of a block-tridiagonal level that the single-column cycle serves with the class records in LDS
 * (AGGMG_OPT_ELEMENT_THREADS, AGGMG_OPT_ELEMENT_RECORDS_LDS) on the same layout: btd_elem_rec_multi_kernel, one thread per
 * element, the level's table of class records copied into LDS once per workgroup, which then walks the columns of the
 * group -- where btd_multi_kernel gives every row a thread and streams the level's full operator arrays.  A half of a
 * level qualifies when the level has blocks of 4 rows with compressed couplings and symmetric packing, an operator
 * dictionary with packed records of at most the cap of AGGMG_OPT_ELEMENT_RECORDS_LDS classes (and the lossless symmetric
 * residual form where the half forms a residual), AGGMG_OPT_ELEMENT_THREADS is on, the half has at least one sweep, and
 * a tile of 256 elements owns something under the half's halo (aggmg_multi_element_tile_plan); every other launch keeps
 * btd_multi_kernel, the levels with blocks of 2 rows and the zero-sweep transfer launches of patch levels among them.
 * Every result is bit for bit the same with the option on or off.  Read at every call.  Off by default: at 2^20 and 2^22
 * fine elements the K-column V(3,3) cycle takes 0.74 - 0.80 of its time with the option on (K = 4, 8), but at 2^12, where
 * the cycle is bound by launches, a workgroup's walk over 8 columns makes it 0.080 -> 0.100 ms
 * (profiles/r37_multi_elem_threads.md).  aggmg_multi_element_thread_launches counts the launches, aggmg_hier_level_multi_element_threads says which halves of a
 * level the kernel would serve.  (The number stands in parentheses for the reason given at option 15.) */
#define AGGMG_OPT_MULTI_ELEMENT_THREADS (16)
int aggmg_set_option(aggmg_ctx* ctx, int option, int value);
/* Launches of the K-column element-thread kernel (AGGMG_OPT_MULTI_ELEMENT_THREADS) on this context so far: one per half,
 * level and group of up to 8 columns.  A counter of its own: aggmg_element_thread_launches,
 * aggmg_element_record_lds_launches and aggmg_replay_launches do not count these launches. */
int aggmg_multi_element_thread_launches(aggmg_ctx* ctx, int64_t* count);
/* Which halves of level `level` of a K-column V(nPre, nPost) cycle the K-column element-thread kernel would serve under
 * the context's options as they stand: *down the descent (nPre sweeps, residual, restriction), *up the ascent
 * (prolongation, nPost sweeps); both 0 on a level that is not block-tridiagonal, on the coarsest one and on a hierarchy
 * whose K-column cycle runs column by column (aggmg_hier_multi_info). */
int aggmg_hier_level_multi_element_threads(aggmg_ctx* ctx, const aggmg_hier* h, int level, int nPre, int nPost, int* down,
                                           int* up);
/* The tile of a K-column element-thread launch (needs no context): a workgroup holds *tile_elems = 256 elements, keeps
 * `halo` of them on either side -- nPre + 1 in a descent, nPost in an ascent -- and owns *owned, a multiple of rho, the
 * agglomeration ratio a descent restricts to (1 for an ascent); 0: no such launch, the half keeps btd_multi_kernel. */
int aggmg_multi_element_tile_plan(int halo, int rho, int* tile_elems, int* owned);
/* Stage launches of the coarsest solve that read their factors from LDS (AGGMG_OPT_COARSE_DICTIONARY) on this context
 * so far: two per chunk stage that took the form and solve (one forward, one backward), whatever the number of columns
 * of the launch. */
int aggmg_coarse_dictionary_launches(aggmg_ctx* ctx, int64_t* count);
/* The cap on classes in force (AGGMG_OPT_COARSE_DICTIONARY; 0: off) and, where max_cap is not NULL, the largest value
 * the option takes. */
int aggmg_coarse_dictionary_cap(aggmg_ctx* ctx, int* cap, int* max_cap);
/* Launches of the element-thread kernels with the class records in LDS (AGGMG_OPT_ELEMENT_RECORDS_LDS) on this context
 * so far. */
int aggmg_element_record_lds_launches(aggmg_ctx* ctx, int64_t* count);
/* The cap on classes in force (AGGMG_OPT_ELEMENT_RECORDS_LDS; 0: off) and, where max_cap is not NULL, the largest value
 * the option takes. */
int aggmg_element_record_lds_cap(aggmg_ctx* ctx, int* cap, int* max_cap);
/* A test and diagnostic hook, not part of what a solver calls: the host repack behind those records (needs no context,
 * no device), exposed so that the record's layout and its precomputed words can be checked without a GPU: rec [nclasses][*words] from the dictionary's
 * arrays of a level with blocks of 4 rows -- bsym [nclasses][10], qrow and qmir [nclasses][4], dup [nclasses][10] and
 * corr [nclasses][4] (both NULL: zeros), lf [nclasses][4] second entries (lf_unit != 0) or [nclasses][4][2] rows.  Word
 * offsets in a record: bsym 0, pcol 10, qrow 14, qmir 18, dup 22, corr 32 (four 32-bit words), rows of L 34.  *words
 * (may be NULL) receives the record's length in doubles, also when nclasses == 0. */
int aggmg_element_record_pack(int nclasses, const double* bsym, const double* qrow, const double* qmir, const double* dup,
                              const uint32_t* corr, const double* lf, int lf_unit, double* rec, int* words);
/* Launches of the element-thread kernel (AGGMG_OPT_ELEMENT_THREADS) on this context so far. */
int aggmg_element_thread_launches(aggmg_ctx* ctx, int64_t* count);
/* Launches of the element-thread two-level kernels (AGGMG_OPT_PAIR_ELEMENT_THREADS) on this context so far. */
int aggmg_pair_element_thread_launches(aggmg_ctx* ctx, int64_t* count);
/* Cycles of aggmg_vcycle_dev that replayed their pre-smoothing (AGGMG_OPT_REPLAY_PRESMOOTH) on this context so far. */
int aggmg_replay_launches(aggmg_ctx* ctx, int64_t* count);
/* Launches of the K-column multiplicative patch sweep kernel (aggmg_smooth_multi_dev, and the patch levels of the
 * K-column cycle under AGGMG_OPT_PATCH_MULTI) on this context so far. */
int aggmg_patch_multi_launches(aggmg_ctx* ctx, int64_t* count);
/* Launches of the K-column hybrid / additive patch sweep kernel (aggmg_smooth_multi_dev on a smoother of
 * aggmg_patch_schwarz_setup, and the hybrid patch levels of the K-column cycle, both under
 * AGGMG_OPT_PATCH_SCHWARZ_MULTI) on this context so far.  aggmg_patch_multi_launches does not count them. */
int aggmg_patch_schwarz_multi_launches(aggmg_ctx* ctx, int64_t* count);
/* Launches of the K-column chain kernel (the chain levels of the K-column cycle under AGGMG_OPT_CHAIN_MULTI) on this
 * context so far. */
int aggmg_chain_multi_launches(aggmg_ctx* ctx, int64_t* count);
/* The tiles of a K-column chain launch (cgt_multi_kernel; needs no context): a launch of nsweeps point-Jacobi sweeps on
 * a group of kb = 1, 2, 4 or 8 columns of a chain level with m = 1, 2 or 4 rows per block holds tile_blocks = 256 / m
 * blocks per workgroup.  restrict_kind: 0 the launch ends with the sweeps (an ascent), 1 residual and restriction to a
 * chain level, 2 residual and restriction to agglomerates of rho blocks.  It keeps halo_left / halo_right blocks on its
 * sides -- nsweeps each, one more each for a residual, one more on the left for a chain restriction, on the right for an
 * agglomerating one -- and owns `owned`, a multiple of rho for an agglomerating restriction (0: no such launch -- another
 * m or kb, nsweeps outside 0 .. 8, halos that fill the tile).  max_sweeps: the most sweeps the K-column cycle puts into
 * one launch; a half-cycle of more keeps the hierarchy column by column. */
int aggmg_chain_multi_tile_plan(int m, int nsweeps, int restrict_kind, int rho, int kb, int* tile_blocks, int* owned,
                                int* halo_left, int* halo_right, int* max_sweeps);
/* Raw device memory owned by the context's device (plumbing for harnesses without torch, and the storage of the
 * Julia shim's DeviceVector).  aggmg_dev_alloc returns ZEROED memory: a fresh vector is the zero initial guess of
 * ldiv! (src/solvers.jl:66,87). */
int aggmg_dev_alloc(aggmg_ctx* ctx, int64_t nbytes, void** out);
int aggmg_dev_free(aggmg_ctx* ctx, void* ptr);
int aggmg_memcpy_h2d(aggmg_ctx* ctx, void* dst_dev, const void* src_host, int64_t nbytes);
int aggmg_memcpy_d2h(aggmg_ctx* ctx, void* dst_host, const void* src_dev, int64_t nbytes);
/* Page-locked host memory for the host-pointer entry points (aggmg_vcycle: what multigrid_v_cycle(H, x0, b) /
 * ldiv!(y, H, b) on host vectors call, src/solvers.jl:19-50,63-92).  Pageable arrays are staged through pinned chunks by
 * worker threads (24 - 28 GB/s); arrays the caller keeps for many calls -- the vectors of a Krylov loop around ldiv! --
 * can be page-locked ONCE instead: copies from and to a registered range are single asynchronous DMA transfers on the
 * context's stream.  aggmg_host_register page-locks an existing range (hipHostRegister; the range must stay valid
 * until aggmg_host_unregister or aggmg_destroy), aggmg_host_alloc hands out pinned memory (hipHostMalloc) that
 * aggmg_host_free returns.  Registering per call does not pay: the registration costs what it saves (measured). */
int aggmg_host_register(aggmg_ctx* ctx, void* ptr, int64_t nbytes);
int aggmg_host_unregister(aggmg_ctx* ctx, void* ptr);
int aggmg_host_alloc(aggmg_ctx* ctx, int64_t nbytes, void** out);
int aggmg_host_free(aggmg_ctx* ctx, void* ptr);

/* ---- operators: H.mStiffness[k], H.mInterpolation[k] (src/mesh_heirarchy.jl:20,26) ---------- */
#define AGGMG_OP_STIFFNESS 0 /* used as A*u only                    src/solvers.jl:33,36,44 */
#define AGGMG_OP_TRANSFER 1  /* used as L*v and L'*v                src/solvers.jl:36,42   */
/* Upload a SparseMatrixCSC (m x n).  The device keeps a row-gather form (CSR, int32 indices)
 * and, for transfers, the transposed orientation too (the CSC arrays as given are the CSR of
 * L').  Index maps are preserved exactly: entry order inside a row/column is ascending, explicit
 * zeros stay stored.  Rejects dimensions or nnz >= 2^31 (AGGMG_ERR_ARGUMENT).  The arrays are validated on the
 * device: a colptr that does not start at the index base, decreases or leaves 0 .. nnz, and row indices not strictly
 * ascending inside a column are AGGMG_ERR_ARGUMENT, a row index outside 0 .. m - 1 is AGGMG_ERR_DIMENSION.  nnz is
 * colptr[n] - base: rowval and nzval must hold that many entries (only the caller knows their lengths). */
int aggmg_csc_upload(aggmg_ctx* ctx, int64_t m, int64_t n, const int64_t* colptr,
                     const int64_t* rowval, const double* nzval, int one_based, int kind,
                     aggmg_op** out);
int aggmg_op_free(aggmg_ctx* ctx, aggmg_op* op);
int aggmg_op_shape(aggmg_ctx* ctx, const aggmg_op* op, int64_t* m, int64_t* n, int64_t* nnz);
/* Read the device index maps back (bit-exactness tests of the transfer index maps).
 * transposed == 0: CSR of the matrix (rowptr[m+1], colind[nnz], vals[nnz]);
 * transposed != 0: CSR of its transpose (rowptr[n+1], ...), transfers only.  0-based int32. */
int aggmg_op_download(aggmg_ctx* ctx, const aggmg_op* op, int transposed, int32_t* rowptr,
                      int32_t* colind, double* vals);
/* No-op, kept for ABI compatibility: the library keeps no host copy of an operator (set-up runs on the device). */
int aggmg_op_release_host(aggmg_ctx* ctx, aggmg_op* op);

/* ---- smoothers: src/smoother.jl ------------------------------------------------------------- */
/* dg_smoother(mesh, A, :blockJac) src/smoother.jl:153-165 and cg_smoother(..., :addSchwarz /
 * :hybridSchwarz) :104-134.  blockinds is the reference's mBlockInds Matrix{Int64}(m x nb),
 * column-major, 1-based when one_based != 0.  Diagonal blocks A[inds,inds] are extracted and
 * factorised with partial pivoting (exact zero pivot -> AGGMG_ERR_SINGULAR naming the block).
 * kind: 0 = BlockJacobi (also AdditiveSchwarz: same apply loop, blocks may overlap),
 *       1 = HybridSchwarz (result divided by the per-node block count, src/smoother.jl:24-46),
 *       2 = red-black block Gauss-Seidel -- EXTENSION, the reference has no Gauss-Seidel smoother
 *           (SURVEY.md D1): one sweep = for colour in (even elements, odd elements):
 *           u_e += alpha B_e^{-1} (b - A u)_e on that colour with the newest u.  V-cycles pre-smooth
 *           in this order and post-smooth in the reverse one.  Needs contiguous blocks and a block-
 *           tridiagonal operator, or the element lists of a CG mesh (below): elements of one colour share
 *           no node (AGGMG_ERR_UNSUPPORTED otherwise); aggmg_smoother_apply on such a smoother applies
 *           its block-diagonal part like kind 0.
 * When blockinds are the element node lists of a CG mesh in mesh order ((p+1) x n, consecutive elements
 * sharing exactly one node, local order [left vertex, right vertex, interior nodes], 2 <= p+1 <= 9) the
 * SWEEPS with the smoother (aggmg_smooth*, V-cycles) run in the fused chain kernel -- the residual of a
 * tile into LDS, then every row its row of A_e \ r_e from the element inverse kept in registers;
 * aggmg_smoother_apply keeps the generic batched-block kernel.  Same results to round-off. */
int aggmg_blockjacobi_setup(aggmg_ctx* ctx, aggmg_op* A, int64_t m, int64_t nb,
                            const int64_t* blockinds, int one_based, int kind,
                            aggmg_smoother** out);
/* dg_smoother / cg_smoother (..., :jac): JacobiSmoother(Diagonal(A)) src/smoother.jl:95-102,146-152 */
int aggmg_jacobi_setup(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother** out);
/* cg_smoother(cgMesh, A, :jac) src/smoother.jl:88-102 with the element node lists the reference's
 * cg_smoother holds in cgMesh.mElements[k].mNodesInd (the (p+1) x n matrix its Schwarz variants store
 * as mBlockInds, src/smoother.jl:104-134): element_nodes is that matrix, column-major, 1-based when
 * one_based != 0, local node order [left vertex, right vertex, interior nodes] (src/cg_mesh.jl:35-45).
 * Same smoother as aggmg_jacobi_setup (Diagonal(A)); when consecutive elements share exactly one node
 * and every stored entry of A couples nodes of one element (true of every CG stiffness matrix and
 * of its Galerkin coarsenings, src/mesh_heirarchy.jl:53-59) the level additionally gets the
 * element-contiguous "chain" form and runs the LDS-tiled fused point-Jacobi kernel
 * (aggmg_smoother_is_structured reports 1).  Vectors stay in the reference's vertices-first
 * numbering (src/cg_mesh.jl:37-45,59-65) at every entry point.  Anything else falls back to the
 * generic CSR kernels with identical results. */
int aggmg_jacobi_setup_elements(aggmg_ctx* ctx, aggmg_op* A, int64_t nodes_per_element, int64_t n_elements,
                                const int64_t* element_nodes, int one_based, aggmg_smoother** out);
/* BlockDiagonal (factorize = 0: apply = `A * X`, mul! src/block_diagonal.jl:166-176) and
 * BlockDiagonalLU (factorize = 1: apply = `A \\ X`, ldiv! :299-309; `lu(A)` :276) as block objects of
 * the same kind as the block smoother: blocks = nb dense m x m blocks, each column-major, with the
 * contiguous index lists the BlockDiagonal(mBlocks) constructor (:27-41) makes.  Applied with
 * aggmg_smoother_apply(..., alpha = 1).  A singular block -> AGGMG_ERR_SINGULAR. */
int aggmg_blockdiag_setup(aggmg_ctx* ctx, int64_t m, int64_t nb, const double* blocks, int factorize,
                          aggmg_smoother** out);
/* EXTENSION: element-patch Schwarz smoother of a DG level -- the arithmetic of HybridSchwarzSmoother /
 * AdditiveSchwarzSmoother (src/smoother.jl:1-46) on lists the call generates itself.  The level has ne elements
 * of m rows, contiguous and aligned (A is (m ne) x (m ne)); the patches are {e, .., e + width - 1},
 * e = 0 .. ne - width (one patch of all elements where ne < width), width = 2, 3 or 4 (anything else:
 * AGGMG_ERR_ARGUMENT).  hybrid != 0: the summed patch corrections of a row are divided by the number of patches
 * covering its element (1 at both ends of the level, `width` well inside); hybrid = 0: added as they are (at
 * alpha = 2/3 that form diverges in a V-cycle: DESIGN.md section 19).
 *   width = 2 on an operator that is block tridiagonal in the element blocking, m = 1 .. 8 in the coupling forms
 * the block-Jacobi set-up produces (compressed 2 .. 8, dense 1 .. 5), ne >= 2: the FUSED form.  The ne - 1 dense
 * patch blocks are assembled on the device from the element blocks, inverted by the kernel of every other block
 * smoother, and kept per row as the two inverse rows the row applies (zeros where a patch does not exist); sweeps
 * run in patch_sweep_kernel -- the tile's iterate and residual in LDS, up to AGGMG_MAX_SWEEP_WEIGHTS sweeps per
 * launch -- with no index list and no CSR operator.  A->btd is set as by a block-Jacobi set-up (aggmg_residual takes
 * the fused residual), and a hierarchy runs the level's transfers in the fused block-tridiagonal launches.
 * MEMORY: the inverse rows take 32 m bytes per row (4 m doubles), i.e. 128 m^2 bytes per element: 8.6 GB at 2^24
 * elements of m = 4; set-up holds the dense blocks and their inverses (another 64 m bytes per row) until it returns.
 * With AGGMG_OPT_OPERATOR_DICTIONARY set, set-up then looks for the classes of bitwise identical per-element records
 * (inverse rows, diagonal block, couplings); where there are at most 1024, the sweeps read one copy of each by a 16-bit
 * class per element -- the same bits, so the same results bit for bit.  More classes: the full arrays, no error.  The
 * full arrays stay allocated in either case.
 *   Everything else -- wider patches, another block size, an operator that is not block tridiagonal -- takes the
 * generic route: the call builds the lists and the smoother aggmg_blockjacobi_setup(kind 0 / 1) makes of them.
 * Same results to round-off; aggmg_smoother_patch_info reports fused = 0.
 * A singular patch -> AGGMG_ERR_SINGULAR naming it (1-based).
 * The smoothed V-cycle is NOT a symmetric preconditioner (the division by the cover counts does not commute with
 * the patch solves): aggmg_pcg_dev is not valid on a hierarchy holding such a level, aggmg_fgmres_dev is.  (The
 * multiplicative sweeps over the same patches, aggmg_patch_gs_setup, give a symmetric cycle.)
 * aggmg_dist_create takes the fused form (ghost widths sized for a reach of two elements per sweep) and refuses the
 * generic route (AGGMG_ERR_UNSUPPORTED). */
int aggmg_patch_schwarz_setup(aggmg_ctx* ctx, aggmg_op* A, int64_t m, int64_t ne, int width, int hybrid,
                              aggmg_smoother** out);
/* width (0: sm is not an element-patch Schwarz smoother), hybrid (1 / 0) and whether sm runs the fused form */
int aggmg_smoother_patch_info(aggmg_ctx* ctx, const aggmg_smoother* sm, int* width, int* hybrid, int* fused);
/* Distinct operator records of the smoother's dictionary (AGGMG_OPT_OPERATOR_DICTIONARY): 0 when sm is not a fused
 * element-patch Schwarz smoother or has no dictionary -- its sweep launches then read the full arrays. */
int aggmg_smoother_patch_dictionary(aggmg_ctx* ctx, const aggmg_smoother* sm, int* nclasses);
/* The tiles of the fused sweep launch on elements of m rows (no device call; tests and tools size their cases with
 * it): a launch of nsweeps sweeps holds tile_elems elements per workgroup, of which it owns `owned` (0: no such
 * launch); runs of more than max_sweeps sweeps are cut into launches of at most that many. */
int aggmg_patch_tile_plan(int m, int nsweeps, int* tile_elems, int* owned, int* max_sweeps);
/* EXTENSION: MULTIPLICATIVE two-colour element-patch smoother of a DG level: the patches
 * P_e = {e, e + 1}, e = 0 .. ne - 2, of aggmg_patch_schwarz_setup's fused form -- the same element blocks, the same
 * inverse rows, the same dictionary records -- applied one colour at a time.  A forward sweep of weight w is the
 * half-sweeps c = 0, 1, each
 *     r = b - A u  (from the current u);   u[P_e] += w inv(A[P_e, P_e]) r[P_e]  for every patch e = c (mod 2)
 * (the patches of a colour are disjoint; an element none of them covers keeps its value); a reverse sweep runs c = 1, 0.
 * aggmg_smooth(_weighted)_dev, aggmg_smoother_solve_dev, aggmg_smoother_apply, aggmg_hier_estimate_lambda_max and the
 * pre-smoothing of a cycle run forward sweeps, the post-smoothing of a cycle reverse ones; a weight schedule applies
 * w_s to both halves of sweep s.  The sweeps run in patch_gs_kernel, up to AGGMG_MAX_SWEEP_WEIGHTS per launch (see
 * aggmg_patch_gs_tile_plan).  With nPre == nPost and the post weights the pre weights reversed, the V-cycle is a
 * SYMMETRIC preconditioner on a symmetric operator: aggmg_pcg_dev is valid on such a hierarchy.
 *   There is no generic route.  AGGMG_ERR_UNSUPPORTED, the message naming the reason, where the fused form does not
 * apply: ne < 2, an operator that is not block tridiagonal in the element blocking, a block size the kernel is not
 * instantiated for (compressed couplings 2 .. 8, dense 1 .. 5).  A singular patch -> AGGMG_ERR_SINGULAR naming it
 * (1-based).  Memory, dictionary, aggmg_smoother_download_blocks, aggmg_smoother_patch_info (width 2, hybrid 0,
 * fused 1), aggmg_smoother_launch_bytes and the refusals of aggmg_dist_create / aggmg_hier_launch_bytes are those of
 * the fused form of aggmg_patch_schwarz_setup; K columns run column by column unless AGGMG_OPT_PATCH_MULTI is set. */
int aggmg_patch_gs_setup(aggmg_ctx* ctx, aggmg_op* A, int64_t m, int64_t ne, aggmg_smoother** out);
/* kind: 0 sm is not an element-patch smoother, 1 additive, 2 hybrid (aggmg_patch_schwarz_setup), 3 multiplicative
 * (aggmg_patch_gs_setup) */
int aggmg_smoother_patch_kind(aggmg_ctx* ctx, const aggmg_smoother* sm, int* kind);
/* The tiles of the multiplicative sweep launch, as aggmg_patch_tile_plan gives the hybrid one's: a launch of nsweeps
 * sweeps holds tile_elems elements per workgroup, keeps `halo` = 2 nsweeps + 1 of them on either side and owns `owned`
 * (0: no such launch); runs of more than max_sweeps sweeps are cut into launches of at most that many. */
int aggmg_patch_gs_tile_plan(int m, int nsweeps, int* tile_elems, int* owned, int* halo, int* max_sweeps);
/* The tiles of the K-column multiplicative sweep launch (patch_gs_multi_kernel; needs no context): a launch of nsweeps
 * sweeps on a group of kb = 1, 2, 4 or 8 columns of a level with m = 2 or 4 rows per element holds tile_elems = 256 / m
 * elements per workgroup, keeps `halo` = 2 nsweeps + 1 of them on either side and owns `owned` (0: no such launch --
 * another m or kb, nsweeps outside 1 .. max_sweeps' range); runs of more than max_sweeps sweeps are cut into launches of
 * at most that many. */
int aggmg_patch_gs_multi_tile_plan(int m, int nsweeps, int kb, int* tile_elems, int* owned, int* halo, int* max_sweeps);
/* The tiles of the K-column hybrid / additive sweep launch (patch_sweep_multi_kernel, AGGMG_OPT_PATCH_SCHWARZ_MULTI;
 * needs no context): the same slab of tile_elems = 256 / m elements for m = 2 or 4 and kb = 1, 2, 4 or 8; a launch of
 * nsweeps sweeps keeps `halo` = 2 nsweeps elements on either side and owns `owned` = tile_elems - 4 nsweeps (0: no such
 * launch -- another m or kb, nsweeps outside 1 .. 8); runs of more than max_sweeps = min(8, tile_elems / 8) sweeps are cut
 * into launches of at most that many. */
int aggmg_patch_schwarz_multi_tile_plan(int m, int nsweeps, int kb, int* tile_elems, int* owned, int* halo, int* max_sweeps);
/* EXTENSION: nsweeps sweeps of a fused multiplicative element-patch smoother (aggmg_patch_gs_setup) on ncols column-major
 * columns (column j of U0, B, U starts ld doubles after column j - 1; ld >= N), device pointers, asynchronous on the
 * context stream.  U0 == NULL: the zero iterate.  weights: one factor per sweep (host array, finite values).
 * reverse = 1: the colour order of post-smoothing.  The columns go in groups of up to 8 through patch_gs_multi_kernel,
 * which reads every row's operator words once per group; runs of more sweeps than one launch takes
 * (aggmg_patch_gs_multi_tile_plan) are cut as aggmg_smooth_dev cuts them.  Column j of U is, bit for bit, what the
 * single-column sweeps give on column j.  With AGGMG_OPT_PATCH_SCHWARZ_MULTI on, the call also serves the fused hybrid
 * and additive smoothers of aggmg_patch_schwarz_setup (width 2, fused) through patch_sweep_multi_kernel
 * (aggmg_patch_schwarz_multi_tile_plan), under the same contract; their sweeps have no direction, so `reverse` is accepted
 * and ignored for them.  AGGMG_ERR_UNSUPPORTED, naming the reason, for any other smoother -- a hybrid / additive one with
 * the option off (the message names the option), an element-patch smoother on the generic route (width 3 or 4, or not
 * fused) -- and for element blocks outside the kernels' coverage (compressed couplings with 2 or 4 rows, dense ones with
 * 2); AGGMG_ERR_ARGUMENT for ld < N, ncols < 1, nsweeps < 0 and U overlapping U0 or B. */
int aggmg_smooth_multi_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* U0, const double* B,
                           int64_t ncols, int64_t ld, const double* weights, int nsweeps, int reverse, double* U);
int aggmg_smoother_free(aggmg_ctx* ctx, aggmg_smoother* sm);
/* apply_smoother(S, B; alpha) -> alpha * (S \ B), B is N x ncols column-major, result in Y.
 * src/smoother.jl:6-18,30-46,56-58,69-81.  Host pointers. */
int aggmg_smoother_apply(aggmg_ctx* ctx, aggmg_smoother* sm, const double* B, int64_t N,
                         int64_t ncols, double alpha, double* Y);
/* 1 when the (operator, smoother) pair was recognised as block-tridiagonal with contiguous
 * aligned element blocks and runs the LDS-tiled fused kernels; 0 = generic CSR path. */
int aggmg_smoother_is_structured(aggmg_ctx* ctx, const aggmg_smoother* sm, int* out);

/* ---- sparse set-up operations on the device ---------------------------
 * The products the reference's hierarchy constructors are made of, on operators that are already in
 * HBM; every result is an ordinary operator (aggmg_op) in CSC form.
 * aggmg_bd_sp_apply: `A * S` for A::BlockDiagonal (bd_sp_matmul / bd_sp_colmul, src/block_diagonal.jl:195-264)
 * or `A \ S` for A::BlockDiagonalLU (bd_sp_solve / bd_sp_colsolve, :314-383) with a sparse S: bd is the block
 * object of aggmg_blockdiag_setup (factorize = 0 / 1).  As in the reference, every column of the result
 * holds ALL m rows of each block its column of S touches (zeros included).  The solve applies the explicit
 * inverse of the pivoted LU (the reference runs getrs per block: equal up to round-off).
 * aggmg_sp_matmul: A * B; aggmg_sp_sub: A - B with numerically-zero results dropped (SparseArrays' `-`,
 * SURVEY.md 9.4); aggmg_op_transpose: the adjoint as an operator of its own.  With them
 *     G_c = L' * G * L,   A_c = C_c - D_c * (M_LU \ G_c)          src/mesh_heirarchy.jl:71-72,79-84,98-103
 * run on the device (agglomerationmultigrid1d_amd.api.MeshHierarchy.from_dg_operators).  One thread
 * per result column, accumulation in SparseArrays' order; columns longer than 128 rows are refused
 * (AGGMG_ERR_UNSUPPORTED).  kind: AGGMG_OP_STIFFNESS or AGGMG_OP_TRANSFER for the result. */
int aggmg_bd_sp_apply(aggmg_ctx* ctx, aggmg_smoother* bd, aggmg_op* S, int kind, aggmg_op** out);
int aggmg_sp_matmul(aggmg_ctx* ctx, aggmg_op* A, aggmg_op* B, int kind, aggmg_op** out);
int aggmg_sp_sub(aggmg_ctx* ctx, aggmg_op* A, aggmg_op* B, int kind, aggmg_op** out);
int aggmg_op_transpose(aggmg_ctx* ctx, aggmg_op* A, int kind, aggmg_op** out);
/* The CSC arrays of an operator (colptr[n+1], rowval[nnz], nzval[nnz], 0-based int32) and the dense blocks
 * of a block smoother / block object ([nb][m][m] row-major: the inverses, or the matrices of a
 * factorize = 0 object): read-back for the parity tests of the set-up products. */
int aggmg_op_download_csc(aggmg_ctx* ctx, const aggmg_op* op, int32_t* colptr, int32_t* rowval, double* nzval);
int aggmg_smoother_download_blocks(aggmg_ctx* ctx, const aggmg_smoother* sm, double* out);
/* Test aid for the size guard of the products above: runs their count -> column-pointer scan on n caller-supplied
 * int32 counts (host array).  The total is formed in 64 bits before anything is scanned or allocated; a result of
 * 2^31 or more entries is refused with AGGMG_ERR_UNSUPPORTED (int32 device indices), *total still set. */
int aggmg_debug_scan_counts(aggmg_ctx* ctx, const int32_t* counts_host, int64_t n, int64_t* total);
/* Measurement aid (tools/exp_coarse.py --calibrate; no reference counterpart): a plain 16-byte streaming kernel on
 * `workgroups` workgroups of 256 threads over device buffers of nbytes -- mode 0 copies src to dst, mode 1 only reads
 * src -- timed with HIP events on the context stream (synchronous); *ms_out = its duration.  The ceiling the
 * coarsest solve's streaming steps (src/solvers.jl:39) are held against in DESIGN.md section 5. */
int aggmg_debug_stream_copy(aggmg_ctx* ctx, void* dst, const void* src, int64_t nbytes, int workgroups, int mode,
                            double* ms_out);
/* Test aid for leaks: the device allocations the library itself holds in this process at the moment -- their number and
 * the bytes asked for -- over all contexts and handles (no context argument, like aggmg_version).  Caller-owned memory
 * is not counted: aggmg_dev_alloc's, and all page-locked host memory.  Either pointer may be NULL. */
int aggmg_debug_device_memory(int64_t* live_allocations, int64_t* live_bytes);

/* ---- fused hot-path operations -------------------------------------------------------------- */
/* nsweeps x  `u += apply_smoother(S, b - A*u; alpha)`   src/solvers.jl:32-35,43-46, :199 */
int aggmg_smooth(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, double* u_inout,
                 const double* b, double alpha, int nsweeps);
/* r = b - A*u                                           src/solvers.jl:33,36,44 */
int aggmg_residual(aggmg_ctx* ctx, aggmg_op* A, const double* u, const double* b, double* r_out);
/* rc = L' * r                                           src/solvers.jl:36 */
int aggmg_restrict(aggmg_ctx* ctx, aggmg_op* L, const double* r, double* rc_out);
/* u += L * uc                                           src/solvers.jl:42 */
int aggmg_prolong_add(aggmg_ctx* ctx, aggmg_op* L, const double* uc, double* u_inout);
/* Device-pointer variants (asynchronous on the context stream).  u_out may equal u_in. */
int aggmg_smooth_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* u_in,
                     const double* b, double alpha, int nsweeps, double* u_out);
/* EXTENSION (no reference counterpart: its smoothing loops damp every sweep by the same alpha, src/solvers.jl:32-35):
 * sweep s of the nsweeps sweeps is damped by w[s] (host array, finite values) -- the launches of aggmg_smooth_dev with
 * the same chunking (fused block-tridiagonal and chain kernels, up to 8 sweeps per launch on banded CSR operators, one
 * sweep per launch otherwise), each launch carrying its slice of w.  A red-black Gauss-Seidel sweep takes one weight for
 * both colours.  w with every entry alpha gives aggmg_smooth_dev's bits. */
int aggmg_smooth_weighted_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* u_in,
                              const double* b, const double* w, int nsweeps, double* u_out);
int aggmg_residual_dev(aggmg_ctx* ctx, aggmg_op* A, const double* u, const double* b,
                       double* r_out);
int aggmg_restrict_dev(aggmg_ctx* ctx, aggmg_op* L, const double* r, double* rc_out);
int aggmg_prolong_add_dev(aggmg_ctx* ctx, aggmg_op* L, const double* uc, double* u_inout);

/* ---- hierarchy: MeshHierarchy + multigrid_v_cycle ------------------------------------------- */
/* Coarsest level `u[n] = A_n \\ rhs[n]` (src/solvers.jl:39; UMFPACK re-factorises per cycle in the
 * reference, here the factorisation is done once at aggmg_hier_create). */
/* Environment variables read when the device solver is planned / launched -- measurement and test knobs, none of
 * them changes a result beyond round-off: AGGMG_CR_TAIL_ROWS, AGGMG_CR_MAX_Q (smaller tail / chunks: the tests run
 * the several-stage plan of > 2^24-row systems at small sizes with them), AGGMG_CR_FILL, AGGMG_CR_MINWG,
 * AGGMG_CR_THREADS (chunk and workgroup size sweeps, tools/exp_coarse_knobs.sh), AGGMG_CR_FUSE_TAIL=1 (boundary
 * system solved by the last-arriving workgroup of the forward launch: measured 5x slower). */
#define AGGMG_COARSE_HOST_BANDED 0 /* banded LU with partial pivoting on the host (D2H, solve, H2D) */
#define AGGMG_COARSE_DEVICE_CR 1   /* block cyclic reduction on the device; error if not applicable */
#define AGGMG_COARSE_EXTERNAL 3    /* no factorisation: the caller solves the coarsest system between
                                      aggmg_vcycle_down_dev and aggmg_vcycle_up_dev (multi-GPU driver) */
#define AGGMG_COARSE_AUTO 2        /* device cyclic reduction when the operator is block-tridiagonal
                                      with well-conditioned pivot blocks, host banded LU otherwise;
                                      where the host banded LU would refuse the operator for its band
                                      (2 kl + ku + 1 rows of band storage above 8e9 bytes: a CG operator of
                                      degree >= 2 in the reference's vertices-first numbering from a few
                                      ten thousand rows on) the element-chain order below is tried first.
                                      Every operator either solver takes today keeps its solver and its bits */
#define AGGMG_COARSE_DEVICE_CHAIN 4 /* the same device cyclic reduction in ELEMENT-CHAIN order: the coarsest
                                      operator is a CG operator whose chain form -- blocks of m = p rows [left
                                      vertex of element e, its interior nodes], block-tridiagonal in that order
                                      -- a chain smoother left on it (aggmg_jacobi_setup_elements, the Schwarz /
                                      Gauss-Seidel set-ups on a CG mesh) or, with AGGMG_OPT_DETECT_CHAIN on, its
                                      pattern shows.  Every solve gathers the right-hand side into block
                                      order, reduces, scatters back: on the context's stream, nothing crosses
                                      PCIe.  Accepted on the same probe (backward error < 1e-10, the product
                                      formed from the operator in ITS numbering, not from the packed blocks).
                                      AGGMG_ERR_UNSUPPORTED with the reason: no chain form, m > 8, a
                                      near-singular pivot block, probe refused.  The phase-by-phase
                                      entry points of the partitioned cycle (aggmg_coarse_plan ...) do not
                                      take such a hierarchy */
/* Mirrors the operator vectors of `struct MeshHierarchy` src/mesh_heirarchy.jl:17-28:
 * stiffness[nlevels], smoothers[nlevels-1] (the coarsest level is solved directly,
 * src/solvers.jl:39), interpolation[nlevels-1] with interpolation[k]: level k+1 -> level k.
 * Level 0 is the finest. */
int aggmg_hier_create(aggmg_ctx* ctx, int nlevels, aggmg_op* const* stiffness,
                      aggmg_smoother* const* smoothers, aggmg_op* const* interpolation,
                      int coarse_mode, aggmg_hier** out);
int aggmg_hier_free(aggmg_ctx* ctx, aggmg_hier* h);
/* multigrid_v_cycle(H, x0, b; nPre, nPost, alpha) -> x    src/solvers.jl:19-50.
 * x0 and b are not modified (src/solvers.jl:25-26); x_out may alias neither.
 * x0 == NULL: a zero initial guess -- ldiv!(H, b) / ldiv!(y, H, b), src/solvers.jl:63-92 -- without a vector of zeros
 * being sent (host form: one transfer less) or read (the finest level then starts from zeros like the others, :29-31);
 * the same bits as passing zeros. */
int aggmg_vcycle(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre,
                 int nPost, double alpha, double* x_out);
int aggmg_vcycle_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre,
                     int nPost, double alpha, double* x_out);
/* multigrid_v_cycle on K right-hand sides (EXTENSION: the reference's methods take vectors, src/solvers.jl:19,63,84).
 * X0, B, X: device, column-major N x ncols, leading dimension ld >= N; X0 == NULL: zero initial guesses (ldiv!).
 * Column j of X is bit for bit what aggmg_vcycle_dev gives for column j of X0 and B.  X must not overlap X0 or B.
 * The columns go in groups (aggmg_hier_multi_info); each non-coarsest level runs one launch per group each way and
 * reads its operator once for the whole group, the coarsest solve runs one launch sequence per group (column by column
 * on the host banded LU and under AGGMG_CR_FUSE_TAIL=1).  A hierarchy with a level
 * the K-column kernel does not cover (CG chain or generic levels, Gauss-Seidel sweeps, agglomerates of different sizes,
 * the preconditioned restriction, block sizes other than 2 / 4 (compressed) and 2 (dense), transfers with other than
 * two coarse modes, sweep counts beyond the tiles' halo) runs aggmg_vcycle_dev column by column instead.  Per-level
 * work space for one group is allocated on the hierarchy on first use (grown for a larger group, freed with it).
 * Asynchronous on the context stream.  AGGMG_ERR_ARGUMENT: NULL, ncols < 1, ld < N, X overlapping X0 or B, negative
 * sweep counts, a hierarchy created with AGGMG_COARSE_EXTERNAL. */
int aggmg_vcycle_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* X0, const double* B, int64_t ncols, int64_t ld,
                           int nPre, int nPost, double alpha, double* X);
/* X = A_n \ B, the coarsest-level direct solve (src/solvers.jl:39) on ncols right-hand sides (EXTENSION: the reference
 * solves vectors); for a one-level hierarchy that is the fine-level `A \ B` behind the err histories (src/solvers.jl:39,120).
 * B, X: device, column-major N_n x ncols (N_n rows of the coarsest operator), leading dimension ld >= N_n.  The
 * columns go in the cycle's groups (aggmg_hier_multi_info); on the device factorisation (block cyclic reduction) a
 * group shares every launch -- forward stages, tail, backward stages, with a grid dimension for the column -- and
 * column j of X is bit for bit the single-column solve of column j (aggmg_vcycle_dev on a one-level hierarchy); on the
 * host banded LU the columns are solved one by one.  Per-column work space for one group is allocated on the hierarchy
 * on first use (grown for a larger group, freed with it).  Asynchronous on the context stream (the host banded LU
 * synchronises, as in aggmg_vcycle_dev).  AGGMG_ERR_ARGUMENT: NULL, ncols < 1, ld < N_n, X overlapping B, a hierarchy
 * created with AGGMG_COARSE_EXTERNAL. */
int aggmg_hier_coarse_solve_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* B, int64_t ncols, int64_t ld, double* X);
/* fused = 1 when the cycle runs K-column launches, 0 when it runs column by column; group = columns per launch */
int aggmg_hier_multi_info(aggmg_ctx* ctx, const aggmg_hier* h, int64_t ncols, int nPre, int nPost, int* fused, int* group);
/* R = B - A X on K columns (EXTENSION: the reference forms residuals of vectors, src/solvers.jl:33,127).  X, B, R:
 * device, column-major N x ncols, leading dimension ld >= N; B == NULL: R = -A X, the bits of a zero B.  Column j of R
 * is bit for bit what aggmg_residual_dev gives for column j.  Block-tridiagonal operators the K-column cycle covers
 * (block sizes 2 / 4 with compressed couplings, 2 with dense ones) run one launch per group of at most 8 columns that
 * reads the operator once for the group; every other operator (CG chain, generic CSR, other block sizes) runs
 * aggmg_residual_dev column by column.  Asynchronous on the context stream.  AGGMG_ERR_ARGUMENT: NULL A, X or R,
 * ncols < 1, ld < N, R overlapping X or B. */
int aggmg_residual_multi_dev(aggmg_ctx* ctx, aggmg_op* A, const double* X, const double* B, int64_t ncols, int64_t ld,
                             double* R);
/* ncycles V-cycles back to back, x <- multigrid_v_cycle(H, x, b): the hot loop of multigrid()
 * (src/solvers.jl:124-126), same arithmetic as ncycles aggmg_vcycle_dev calls.  On block-
 * tridiagonal fine levels the post-smoothing of one cycle and the pre-smoothing of the next run in
 * one fused launch, so the fine operator is read once per cycle instead of twice. */
int aggmg_vcycles_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int ncycles,
                      int nPre, int nPost, double alpha, double* x_out);
/* How the fused descent forms the restricted residual L'(rhs - A u) of src/solvers.jl:36.
 * AGGMG_RESTRICT_EXPLICIT (the default of every hierarchy): r = rhs - A u with the operator's own
 * entries, then L' r -- the reference's arithmetic.  AGGMG_RESTRICT_PRECONDITIONED: (L'D) w from the
 * preconditioned residual w = B^{-1} r that the sweeps already hold; equal in exact arithmetic and
 * ~20 % cheaper per V-cycle (the descent reads neither the diagonal blocks nor L), but w carries the
 * rounding of the stored block inverses.  Measured on the model problem: the factor by which one
 * V(3,3) cycle multiplies the smoothest mode grows like n^2 in every implementation -- reference-
 * order arithmetic 0.002 / 0.031 / 0.498 at 2^20 / 2^22 / 2^24 fine elements, the explicit form the
 * same to three digits, the preconditioned form 0.009 / 0.134 / 2.13: at 2^24 it AMPLIFIES the mode
 * and the multigrid iteration diverges (tests/manual/exp_smooth_mode.py).
 * aggmg_hier_set_restriction therefore returns AGGMG_ERR_UNSUPPORTED for the preconditioned form on
 * hierarchies with more than AGGMG_RESTRICT_PRECONDITIONED_MAX_ELEMS fine elements (where the
 * extrapolated factor passes ~0.05).  No environment variable selects the mode. */
#define AGGMG_RESTRICT_EXPLICIT 0
#define AGGMG_RESTRICT_PRECONDITIONED 1
#define AGGMG_RESTRICT_PRECONDITIONED_MAX_ELEMS (1 << 21)
int aggmg_hier_set_restriction(aggmg_ctx* ctx, aggmg_hier* h, int mode);
int aggmg_hier_get_restriction(aggmg_ctx* ctx, const aggmg_hier* h, int* mode);
/* The two halves of the V-cycle around the coarsest solve (src/solvers.jl:28-37 and :41-47), for
 * callers that solve the coarsest system themselves (element-partitioned multi-GPU runs gather it
 * across ranks).  After _down the coarsest right-hand side is in the buffer reported by
 * aggmg_hier_coarse_buffers(); _up expects the coarsest solution in the solution buffer. */
int aggmg_vcycle_down_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre,
                          double alpha);
int aggmg_vcycle_up_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, int nPost, double alpha,
                        double* x_out);
/* The ascent in three calls so that a partitioned run can exchange the interface elements of
 * x_out while the rest of the fine level is still being smoothed: part 0 = the coarser levels,
 * part 1 = the fine-level tiles holding elements [0, head_elems) and [tail_elem, ne), part 2 = the
 * remaining fine-level tiles.  Parts 1 and 2 do not depend on each other (they may be issued on
 * different streams, aggmg_set_stream); together they are bitwise aggmg_vcycle_up_dev.
 * Offered where the fine level runs the fused block-tridiagonal kernel, and where it is a multiplicative element-patch
 * level (aggmg_patch_gs_setup) with a structured transfer of one ratio and 1 <= nPost <= the sweeps of one launch
 * (aggmg_patch_gs_tile_plan's max_sweeps): parts 1 and 2 are then one launch each that prolongs and sweeps its tiles.
 * AGGMG_ERR_UNSUPPORTED, with nothing launched, everywhere else -- hybrid patch levels, agglomerates of different sizes,
 * chunked sweep counts, nPost == 0 (aggmg_vcycle_up_split_ok answers beforehand).  part 3: the finest level alone,
 * every tile, whatever kernel runs it (after the coarser levels went through part 0 or aggmg_vcycle_up_coarse_dev). */
int aggmg_vcycle_up_split_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, int nPost, double alpha,
                              double* x_out, int64_t head_elems, int64_t tail_elem, int part);
/* *ok = 1 where parts 0 - 2 of aggmg_vcycle_up_split_dev exist for this hierarchy and nPost, else 0 */
int aggmg_vcycle_up_split_ok(aggmg_ctx* ctx, const aggmg_hier* h, int nPost, int* ok);
/* The ascent below the finest level in two parts around the exchange of the coarsest solution's ghost blocks
 * (element-partitioned runs; src/solvers.jl:41-47 for the levels between the coarsest and the finest): part 2 runs the
 * tiles of the first launch that read none of the first ghosts_lo / last ghosts_hi elements of the coarsest level -- they
 * can go while the neighbours' blocks are still travelling --, part 1 the remaining tiles at the two ends and the rest of
 * those levels.  Both parts together = aggmg_vcycle_up_split_dev(part 0), bit for bit.  AGGMG_ERR_UNSUPPORTED unless
 * the levels below the finest are one two-level launch next to the coarsest level (aggmg_hier_level_paired). */
int aggmg_vcycle_up_coarse_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, int nPost, double alpha, int part,
                               int64_t ghosts_lo, int64_t ghosts_hi);
int aggmg_hier_coarse_buffers(aggmg_ctx* ctx, aggmg_hier* h, void** rhs_dev, void** sol_dev,
                              int64_t* n);
/* The device coarsest solve phase by phase, for element-partitioned runs: block cyclic reduction
 * eliminates the first `chunk_log2` levels independently per chunk of 2^chunk_log2 block rows, so
 * every rank runs `chunk_forward` on the chunks of its own block range [blk_lo, blk_hi) (aligned to
 * the chunk size) from its owned right-hand side, the ranks exchange their slices of the two
 * boundary vectors partR / partL (n_boundary * block_size values each, written at global positions),
 * every rank solves the small boundary system, and `chunk_backward` produces the owned solution.
 * aggmg_coarse_plan reports chunk_log2 = -1 when the hierarchy's coarsest solver has no such plan. */
int aggmg_coarse_plan(aggmg_ctx* ctx, const aggmg_hier* h, int* chunk_log2, int64_t* n_boundary,
                      int* block_size, int64_t* n_blocks);
int aggmg_coarse_chunk_forward_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* rhs_owned, int64_t blk_lo,
                                   int64_t blk_hi, double* partR, double* partL);
int aggmg_coarse_boundary_solve_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* partR, const double* partL,
                                    double* xq);
int aggmg_coarse_chunk_backward_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* rhs_owned, int64_t blk_lo,
                                    int64_t blk_hi, const double* xq, double* x_owned);
/* Which kernels smooth a level (level 0 = finest): the fused block-tridiagonal kernel (DG /
 * agglomerated levels), the fused chain kernel (CG levels set up with aggmg_jacobi_setup_elements),
 * the generic CSR kernels, or -- last level -- the coarsest direct solve. */
#define AGGMG_LEVEL_GENERIC 0
#define AGGMG_LEVEL_FUSED_BTD 1
#define AGGMG_LEVEL_FUSED_CHAIN 2
#define AGGMG_LEVEL_COARSEST 3
int aggmg_hier_level_kind(aggmg_ctx* ctx, const aggmg_hier* h, int level, int* kind);
/* Whether aggmg_vcycle_dev runs levels `level` and `level + 1` in ONE launch each way (nsweeps sweeps per level):
 * small agglomerated levels -- block size 2, dense off-diagonal blocks, one agglomeration ratio per level -- below
 * the finest one, both halves of src/solvers.jl:28-37 / :41-47 for two levels with the hand-over in LDS; bit for bit
 * the separate launches.  The launch is then attributed to `level` (profile tags, aggmg_hier_launch_bytes of both
 * levels apply).  AGGMG_OPT_PAIR_LEVELS switches the pairing off.
 * aggmg_hier_level_paired answers for the descent, aggmg_hier_level_paired_up for the ascent: besides the level
 * kinds the launch needs a tile that holds both levels with their halos, which depends on the two agglomeration
 * ratios, the sweeps and the direction (ratios (16, 16) at three sweeps: no descent tile, an ascent tile); levels
 * without one take one launch each. */
int aggmg_hier_level_paired(aggmg_ctx* ctx, const aggmg_hier* h, int level, int nsweeps, int* paired);
int aggmg_hier_level_paired_up(aggmg_ctx* ctx, const aggmg_hier* h, int level, int nsweeps, int* paired);
/* Whether level `level`'s fused kernel forms its explicit residual from the lossless symmetric form of the operator's
 * entries (AGGMG_OPT_SYMMETRIC_RESIDUAL): 1 when it was built at set-up, 0 otherwise. */
int aggmg_hier_level_sym_residual(aggmg_ctx* ctx, const aggmg_hier* h, int level, int* on);
/* Distinct operator records of the level's dictionary (AGGMG_OPT_OPERATOR_DICTIONARY; a fused level's, a chain level's
 * or the one the two-level launches read); 0: the level has none and its
 * launches read the full arrays. */
int aggmg_hier_level_dictionary(aggmg_ctx* ctx, const aggmg_hier* h, int level, int* nclasses);
/* Sweep-weight schedule of a level (EXTENSION: the reference damps every sweep of every level by the same alpha,
 * src/solvers.jl:19-50).  pre / post: host arrays; afterwards the level's i-th pre-smoothing sweep is damped by pre[i]
 * and its i-th post-smoothing sweep by post[i] in EVERY entry point that runs the cycle on this hierarchy -- aggmg_vcycle
 * (_dev), aggmg_vcycles_dev, aggmg_multigrid_dev, aggmg_pcg_dev, the _multi_ forms, aggmg_vcycle_down_dev / _up_dev --
 * in place of their alpha argument; levels without a schedule keep alpha.  A red-black Gauss-Seidel level takes one
 * weight per sweep (both colours).  npre = npost = 0 clears the level.  The weights ride in the kernel arguments of the
 * launches the unscheduled cycle runs (a launch that post-smooths one cycle and pre-smooths the next takes post ++
 * pre), so a schedule whose weights all equal alpha gives the unscheduled bits.
 * AGGMG_ERR_ARGUMENT: NULL, a level outside 0 .. nlevels - 2 (the coarsest level is solved, not smoothed), a count
 * outside 0 .. AGGMG_MAX_SWEEP_WEIGHTS, a weight that is not finite.  A cycle whose nPre / nPost differs from npre /
 * npost of a scheduled level returns AGGMG_ERR_ARGUMENT: nothing is truncated or padded.  aggmg_dist_vcycle_dev refuses
 * a hierarchy that has a schedule (AGGMG_ERR_UNSUPPORTED).  With pcg the cycle is a symmetric preconditioner only when
 * post is pre reversed: that is the caller's responsibility.
 * aggmg_hier_get_sweep_weights: pre / post receive the schedule (room for AGGMG_MAX_SWEEP_WEIGHTS each), *npre = *npost
 * = 0 on a level without one. */
#define AGGMG_MAX_SWEEP_WEIGHTS 8 /* most weights per half: every kernel family fuses at most 8 sweeps per launch */
int aggmg_hier_set_sweep_weights(aggmg_ctx* ctx, aggmg_hier* h, int level, const double* pre, int npre,
                                 const double* post, int npost);
int aggmg_hier_get_sweep_weights(aggmg_ctx* ctx, const aggmg_hier* h, int level, double* pre, int* npre, double* post,
                                 int* npost);
/* Largest eigenvalue of S^-1 A of a level by power iteration, on the device (EXTENSION; what a Chebyshev schedule is
 * scaled by).  v0: device start vector of the level's length, or NULL for a fixed seeded one.  One step is w = S^-1 (A v)
 * -- the operator launch, then one sweep of the level's smoother with factor 1 from the zero iterate --, the estimate
 * ||w|| / ||v|| and v = w / ||w||; iters >= 1 steps, ONE host read at the end (synchronises).  The estimate approaches
 * the eigenvalue from below (0.989 - 0.995 of it after 40 steps on the benchmark hierarchies). */
int aggmg_hier_estimate_lambda_max(aggmg_ctx* ctx, aggmg_hier* h, int level, const double* v0, int iters,
                                   double* lambda_max);
/* The coarsest solve's dictionary (AGGMG_OPT_COARSE_DICTIONARY).  *nstages: the chunk stages of the device solve (0: none,
 * or no device solve).  For stage s < *nstages: taken[s] 1 when its launches read their factors from LDS, first_level[s]
 * and nlevels[s] the reducing levels it spans.  For reducing level l: even_classes[l] / odd_classes[l], the distinct
 * records found among its even rows' multipliers / its odd rows' factors; -1 where set-up did not class the level (the
 * option off, another block size, a level of the tail, a level behind the first one of its stage that went over the
 * cap), 0 where there are more than the search tracks (1024).  Every array holds `capacity` entries, at least 40;
 * entries beyond the stages / levels are 0 / -1. */
int aggmg_hier_coarse_dictionary(aggmg_ctx* ctx, const aggmg_hier* h, int capacity, int* nstages, int* taken,
                                 int* first_level, int* nlevels, int* even_classes, int* odd_classes);
/* Which coarsest solver a hierarchy uses: on_device (1 = cyclic reduction), its block size and the
 * largest pivot-block condition estimate met while factoring (0 for the host solver). */
int aggmg_hier_coarse_info(aggmg_ctx* ctx, const aggmg_hier* h, int* on_device, int* block_size,
                           double* cond_est);
/* The cyclic reduction pivots inside its m x m blocks only, the reference's `A_n \ rhs_n` (UMFPACK,
 * src/solvers.jl:39) across the whole matrix.  aggmg_hier_create therefore accepts a device factorisation on
 * evidence: it solves one probe system d = A w (w hash-random) and keeps the factorisation only when
 * ||d - A x|| / ||d|| < 1e-10; otherwise AGGMG_COARSE_AUTO falls back to the host banded LU with partial
 * pivoting (AGGMG_COARSE_DEVICE_CR: AGGMG_ERR_UNSUPPORTED).  backward_error receives the probe's figure
 * (-1 when no device factorisation was attempted). */
int aggmg_hier_coarse_probe(aggmg_ctx* ctx, const aggmg_hier* h, double* backward_error);
/* Is the device factorisation one of the element-chain order (AGGMG_COARSE_DEVICE_CHAIN, or AGGMG_COARSE_AUTO on an
 * operator whose band the host solver refuses)?  *on = 1 / 0, *m = rows per block (the degree p), *blocks = elements + 1
 * (the trailing identity-padded block holds the last vertex); 0 / 0 / 0 otherwise.  aggmg_hier_coarse_info, _probe and
 * _tail report this factorisation like any other: on_device 1, block_size m. */
int aggmg_hier_coarse_chain(aggmg_ctx* ctx, const aggmg_hier* h, int* on, int* m, int64_t* blocks);
/* How the device solve ends: the boundary system its chunk stages leave (or the whole system when it is small) goes to
 * ONE workgroup -- *kind = 2: parallel cyclic reduction (block sizes 1 and 2, up to 1024 blocks -- above 512 with one
 * ordinary reduction level around it; kept only where
 * aggmg_hier_create measured it as accurate as kind 1 on a system with a large smooth solution), 1: the register-blocked
 * cyclic reduction of the stages, 0: no device factorisation; *blocks = block rows of that system. */
int aggmg_hier_coarse_tail(aggmg_ctx* ctx, const aggmg_hier* h, int* kind, int64_t* blocks);
/* Milliseconds the last aggmg_vcycle* call spent in the coarsest direct solve (host path:
 * D2H + solve + H2D, measured with the host clock). */
int aggmg_hier_last_coarse_ms(aggmg_ctx* ctx, const aggmg_hier* h, double* ms);

/* Up to four strided 2-D copies of device doubles in ONE launch:
 * dst[g][i * dst_ld[g] + j] = src[g][i * src_ld[g] + j], i < rows[g], j < cols[g].  Packs / unpacks
 * the interface DoFs around the all-gathers of an element-partitioned run (the reference has no
 * counterpart: it is single-process). */
int aggmg_copy_segments_dev(aggmg_ctx* ctx, int nseg, const double* const* src, double* const* dst,
                            const int64_t* rows, const int64_t* cols, const int64_t* src_ld,
                            const int64_t* dst_ld);

/* ---- element-partitioned V-cycle inside the library (BASELINE config 4) -----------
 * The reference is single-process; this is one rank's share of multigrid_v_cycle (src/solvers.jl:19-50)
 * on a LOCAL hierarchy (owned elements + W_k ghost elements per side and level, created with
 * AGGMG_COARSE_EXTERNAL) plus a one-level hierarchy holding the GLOBAL coarsest operator, with the
 * interface exchanges issued by the library on the context's stream: per cycle one all-gather of the
 * interface elements of x0, and the coarsest solve across ranks (chunk elimination on the rank's own
 * block range, all-gather of the chunk-boundary system, replicated boundary solve, back substitution,
 * all-gather of the coarse ghost blocks; small coarsest levels: all-gather of the owned right-hand
 * side + replicated solve).  Layout arrays have nlevels entries (level 0 finest): owned element range
 * [own_lo, own_hi), local range [loc_lo, loc_hi) (owned + ghosts, clipped to the domain), global
 * element counts ne, DoFs per element m, ghost widths W.  Vectors are LOCAL (loc range) device vectors.
 * Owned results are bitwise those of the single-GPU cycle (tests/test_distributed_gpu.py).
 *   Element-patch levels (aggmg_patch_schwarz_setup's fused form, aggmg_patch_gs_setup) are accepted: their sweeps
 * reach 2 S elements per side (multiplicative: 2 S + 1), which the caller's ghost widths must cover -- aggmg_dist_vcycle_dev
 * checks W against its sweep counts before the first launch on a hierarchy that has such a level and returns
 * AGGMG_ERR_UNSUPPORTED ("ghost layers too thin") otherwise.  aggmg_dist_create refuses, with AGGMG_ERR_UNSUPPORTED and
 * the reason in the message: a patch smoother on the generic route, patches wider than two elements, a patch level
 * whose W cannot carry one sweep of its smoother (W < 2, multiplicative: W < 3 -- no smoothed cycle would ever pass the
 * check above), and a multiplicative patch level whose loc_lo is odd (its colours are the parity of the LOCAL element
 * index). */
typedef struct aggmg_dist aggmg_dist;
int aggmg_dist_create(aggmg_ctx* ctx, aggmg_hier* local, aggmg_hier* coarse_global, int world, int rank, int nlevels,
                      const int64_t* own_lo, const int64_t* own_hi, const int64_t* loc_lo, const int64_t* loc_hi,
                      const int64_t* ne, const int32_t* m, const int32_t* W, aggmg_dist** out);
int aggmg_dist_free(aggmg_ctx* ctx, aggmg_dist* d);
/* Collectives, one of:
 *  - RCCL inside the library: rank 0 calls aggmg_rccl_unique_id, the AGGMG_RCCL_ID_BYTES bytes travel to
 *    every rank by any means (they are not secret and small), every rank calls aggmg_dist_init_rccl
 *    (ncclCommInitRank; collective).  librccl.so.1 is loaded with dlopen on first use -- the copy already
 *    in the process if there is one.  nranks_out receives what the communicator reports.  Handing over TWO ids back
 *    to back (nbytes = 2 * AGGMG_RCCL_ID_BYTES, two calls of aggmg_rccl_unique_id) gives the second stream -- the
 *    interface exchange issued under the fine-level ascent -- a communicator of its own: operations of one
 *    communicator in flight on two streams may start in a different order on different ranks and wait for each other.
 *  - a caller-supplied all-gather: recv_dev[r * count + i] = rank r's send_dev[i], ordered on hip_stream
 *    after everything enqueued there so far; returns 0 on success.  ALIASING: the chunk-boundary system is gathered
 *    IN PLACE -- send_dev == recv_dev + rank * count (the caller's own slice of the receive buffer, already in its
 *    final position) -- and the callback has to treat that as an in-place all-gather (ncclAllGather does by
 *    definition; MPI needs MPI_IN_PLACE; a copy-based implementation must not clobber or re-copy that slice).  The
 *    other gathers pass disjoint buffers.
 *  - a device-local loop-back (every slot receives the caller's own data): rehearsals of one rank's
 *    share on a single GPU, measurement only. */
#define AGGMG_RCCL_ID_BYTES 128
typedef int (*aggmg_allgather_fn)(void* user, const double* send_dev, double* recv_dev, int64_t count, void* hip_stream);
int aggmg_rccl_unique_id(aggmg_ctx* ctx, void* id_out, int nbytes);
/* Whether RCCL can be loaded in this process (no context, no device needed): AGGMG_OK, or AGGMG_ERR_UNSUPPORTED
 * with the loader's message copied into why (NUL-terminated, at most nbytes; may be NULL) -- the same outcome
 * aggmg_rccl_unique_id / aggmg_dist_init_rccl report, so that all ranks can agree on a fallback before the first
 * collective.  The environment variable AGGMG_RCCL_LIB names another library file to load (tests). */
int aggmg_rccl_available(char* why, int nbytes);
int aggmg_dist_init_rccl(aggmg_ctx* ctx, aggmg_dist* d, const void* id, int nbytes, int* nranks_out);
int aggmg_dist_set_allgather(aggmg_ctx* ctx, aggmg_dist* d, aggmg_allgather_fn fn, void* user);
/* Neighbour messages.  An interface exchange moves a rank's first / last owned elements into the ghost elements of
 * its left / right neighbour; as grouped ncclSend / ncclRecv between the vectors themselves that is ONE launch
 * with no pack, all-gather or unpack around it (SURVEY.md 8e names it as the equivalent of the interface
 * all-gather).  RCCL and the loop-back do so by default; a caller-supplied collective backend does when it also
 * supplies aggmg_dist_set_sendrecv: fn posts nops operations -- is_send[i] ? send count[i] doubles at dev_ptr[i]
 * to rank peer[i] : receive them from it -- ordered on hip_stream, messages between one pair of ranks matched in
 * order, returns 0 on success (`user` is the pointer given to aggmg_dist_set_allgather).  The environment variable
 * AGGMG_DIST_P2P=0 keeps every exchange on pack -> all-gather -> unpack.
 * aggmg_dist_set_neighbor_layout: the slices [off, off + len) of a local level-`level` vector (finest or
 * coarsest) that go to / are filled from the left and right neighbour, at most two per direction; rank r's
 * to_right must match rank r + 1's from_left slice by slice, to_left rank r - 1's from_right.  Levels with
 * element-contiguous DoFs have it by default; a level given an explicit aggmg_dist_set_exchange_layout loses the
 * default and exchanges by all-gather until this is called. */
typedef int (*aggmg_sendrecv_fn)(void* user, int nops, const int* peer, const int* is_send, double* const* dev_ptr,
                                 const int64_t* count, void* hip_stream);
int aggmg_dist_set_sendrecv(aggmg_ctx* ctx, aggmg_dist* d, aggmg_sendrecv_fn fn);
int aggmg_dist_set_neighbor_layout(aggmg_ctx* ctx, aggmg_dist* d, int level, int nto_left, const int64_t* to_left_off,
                                   const int64_t* to_left_len, int nto_right, const int64_t* to_right_off,
                                   const int64_t* to_right_len, int nfrom_left, const int64_t* from_left_off,
                                   const int64_t* from_left_len, int nfrom_right, const int64_t* from_right_off,
                                   const int64_t* from_right_len);
int aggmg_dist_set_loopback(aggmg_ctx* ctx, aggmg_dist* d);
/* Interface layout of a level whose DoFs are not contiguous per element (a CG level in the reference's
 * vertices-first numbering, src/cg_mesh.jl:37-45,59-65: the interface is a slice of the vertex part plus
 * a slice of the interior part).  count doubles per rank travel; send_*: slices [src, src + len) of the local
 * vector packed at dst of this rank's part; left_* / right_*: slices of the left / right neighbour's part
 * unpacked at dst of the local vector.  level: 0 (finest) or nlevels - 1 (coarsest).  Levels with contiguous
 * elements need no call (first / last W elements, the default). */
int aggmg_dist_set_exchange_layout(aggmg_ctx* ctx, aggmg_dist* d, int level, int64_t count, int nsend,
                                   const int64_t* send_src, const int64_t* send_dst, const int64_t* send_len,
                                   int nleft, const int64_t* left_src, const int64_t* left_dst, const int64_t* left_len,
                                   int nright, const int64_t* right_src, const int64_t* right_dst,
                                   const int64_t* right_len);
/* One all-gather through the configured backend (count doubles per rank); also the smoke test of it. */
int aggmg_dist_allgather_dev(aggmg_ctx* ctx, aggmg_dist* d, const double* send_dev, double* recv_dev, int64_t count);
/* Fill the ghost entries of a local finest- or coarsest-level vector from the neighbours' owned
 * interface elements (needed once for the right-hand side; the cycle does it for x0 itself). */
int aggmg_dist_exchange_ghosts_dev(aggmg_ctx* ctx, aggmg_dist* d, double* x_local, int level);
/* One V-cycle.  x0's ghost entries are overwritten with the neighbours' values unless
 * AGGMG_DIST_X0_GHOSTS_VALID; b must be valid on the whole local range; on return the owned part of
 * x_out is the result (its ghosts are not).  AGGMG_DIST_OVERLAP_NEXT: the caller will pass x_out as the
 * next cycle's x0 (the loop of multigrid, src/solvers.jl:124-126) -- the fine-level ascent then produces
 * the interface elements first and their all-gather runs on a second stream under the rest of that
 * launch; the next call only waits for it.  Same arithmetic either way. */
#define AGGMG_DIST_X0_GHOSTS_VALID 1
#define AGGMG_DIST_OVERLAP_NEXT 2
/* AGGMG_DIST_GRAPH: replay the cycle as a hipGraph.  The first call with a given argument tuple is
 * issued launch by launch, the second is captured (both streams, the collective included) and every
 * later one is a single hipGraphLaunch.  Falls back to launch-by-launch issue for good when the capture
 * fails (a collective backend that cannot be captured), with caller-supplied collectives, the host
 * coarsest solver, or while the event profiler is on.  aggmg_dist_graph_info reports what happened. */
#define AGGMG_DIST_GRAPH 4
int aggmg_dist_vcycle_dev(aggmg_ctx* ctx, aggmg_dist* d, double* x0, const double* b, double* x_out, int nPre,
                          int nPost, double alpha, int flags);
/* exchanges: all-gathers issued so far; chunked: 1 when the coarsest solve follows the partition;
 * backend: 0 none, 1 caller-supplied, 2 RCCL, 3 loop-back */
/* Whether the exchange of the coarsest solution's ghost blocks runs on the side stream under the middle tiles of the
 * two-level ascent (aggmg_vcycle_up_coarse_dev) instead of in front of it.  Off by default (environment
 * AGGMG_DIST_COARSE_OVERLAP=1 makes it the default): it trades an extra launch and two stream joins for the latency of one
 * neighbour exchange, which pays only where that latency is real -- callers time both (bench.py does, in its warm-up) and
 * must choose the same on every rank.  Same results bit for bit either way. */
int aggmg_dist_set_coarse_overlap(aggmg_ctx* ctx, aggmg_dist* d, int on);
int aggmg_dist_info(aggmg_ctx* ctx, const aggmg_dist* d, int64_t* exchanges, int* chunked, int* backend);
int aggmg_dist_graph_info(aggmg_ctx* ctx, const aggmg_dist* d, int64_t* replays, int* captured, int* broken);

/* ---- outer solver loops, device-resident -------------------------------------- */
/* x . y and ||x||_2 of device vectors (fixed reduction tree: reproducible run to run). */
int aggmg_dot_dev(aggmg_ctx* ctx, const double* x, const double* y, int64_t n, double* out);
int aggmg_norm2_dev(aggmg_ctx* ctx, const double* x, int64_t n, double* out);
/* ||b - A x||_2: the `la.norm( A * x - b, 2 )` of src/solvers.jl:129 and :204. */
int aggmg_residual_norm_dev(aggmg_ctx* ctx, aggmg_op* A, const double* x, const double* b, double* out);
/* multigrid(H, x0, b, maxiter, tol) -> x, iter, res, err       src/solvers.jl:116-139:
 * x <- multigrid_v_cycle(H, x, b) until ||A x - b|| < tol ||b|| (:131) or maxiter cycles.  The residual is checked
 * every `check_every` cycles (1 = the reference's loop; c > 1 runs c cycles per check through aggmg_vcycles_dev);
 * res_hist (host, >= ceil(maxiter / check_every) entries) receives one norm per check.
 * The reference's `err` history -- err[i] = ||x_i - u_exact||_2 with u_exact = H.mStiffness[1] \ b (:120, :128) --
 * is formed on the device when u_exact (device vector) and err_hist (host, as long as res_hist) are given: the
 * caller solves the fine system ONCE (a one-level hierarchy of the fine operator is the direct solve: block cyclic
 * reduction when the operator is block-tridiagonal, host banded LU otherwise -- aggmg_hier_create with nlevels = 1)
 * and no iterate crosses PCIe.  Both NULL: no error history.  All vectors are device pointers; x_out may alias
 * neither x0 nor b. */
int aggmg_multigrid_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int maxiter,
                        double tol, int check_every, int nPre, int nPost, double alpha, double* x_out,
                        double* res_hist, int* n_cycles, int* n_checks, const double* u_exact, double* err_hist);
/* iterative_smoother_solve(A, smoother, x0, b; maxiter, tol, alpha) -> x, iter, res, err
 * src/solvers.jl:189-213; same conventions as above (u_exact = A \ b of :194, err[i] of :202). */
int aggmg_smoother_solve_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* x0,
                             const double* b, int maxiter, double tol, double alpha, int check_every,
                             double* x_out, double* res_hist, int* n_iters, int* n_checks, const double* u_exact,
                             double* err_hist);
/* Conjugate gradients on A x = b with ldiv!(y, H, r) (one V-cycle from a zero guess,
 * src/solvers.jl:84-92) as the preconditioner; x_inout holds the initial guess and the result.
 * EXTENSION: the reference provides ldiv! so that a hierarchy can be used as a preconditioner but
 * has no Krylov loop of its own.  Needs A symmetric positive definite and nPre == nPost.
 * res_hist (host, >= maxiter entries): ||r|| of the recurrence after every iteration. */
int aggmg_pcg_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, double* x_inout, int maxiter, double tol,
                  int nPre, int nPost, double alpha, double* res_hist, int* n_iters);
/* ---- flexible GMRES around the cycle (EXTENSION: the reference has no Krylov loop).  aggmg_pcg_dev needs a symmetric
 * cycle and checks nothing: with nPre != nPost, a sweep-weight schedule whose post half is not the pre half reversed, a
 * hybrid Schwarz or Gauss-Seidel level with unequal counts, it returns a wrong answer.  A minimal-residual method is
 * valid for every cycle. ---- */
/* The two streaming passes of its orthogonalisation, over a device basis V (column-major, vector i at V + i * ld,
 * ld >= n, 1 <= nvec <= AGGMG_FGMRES_MAX_RESTART + 1) and a device vector w.  Both synchronous.
 * aggmg_multi_dot_dev: out_host[i] = V_i . w, i < nvec, with ONE pass over w per group of 8 vectors; entry i is bit
 * for bit aggmg_dot_dev(V_i, w, n).
 * aggmg_multi_axpy_norm_dev: w[r] <- fma(c[nvec-1], V_{nvec-1}[r], ... fma(c[0], V_0[r], w[r])) for r < n (ascending i,
 * in place, groups of 8, one pass over w per group; rows >= n are not touched); *norm_out_host (may be NULL) receives
 * ||w||_2 of the stored vector, summed by the pass that stores it: bit for bit aggmg_norm2_dev(w, n) afterwards.
 * Fixed slices and summation trees, no atomics: the same bits run to run.  AGGMG_ERR_ARGUMENT: NULL, n < 0, nvec
 * outside 1 .. 65, ld < n, w overlapping V. */
int aggmg_multi_dot_dev(aggmg_ctx* ctx, const double* V, int64_t n, int64_t nvec, int64_t ld, const double* w,
                        double* out_host);
int aggmg_multi_axpy_norm_dev(aggmg_ctx* ctx, const double* V, int64_t n, int64_t nvec, int64_t ld, const double* coef_host,
                              double* w_inout, double* norm_out_host);
/* Right-preconditioned flexible GMRES(restart) on A x = b with one V-cycle from a zero guess as M^-1
 * (aggmg_vcycle_dev(h, NULL, v, ...): sweep-weight schedules apply as in every other solver); x_inout holds the initial
 * guess and the result.  Classical Gram-Schmidt, one pass, no re-orthogonalisation.  Per iteration j of a restart cycle:
 * z_j = M^-1 v_j, w = A z_j, h = V' w (aggmg_multi_dot_dev's pass), w -= V h and h_{j+1,j} = ||w|| (aggmg_multi_axpy_norm_dev's
 * pass), one read-back of the column, v_{j+1} = w / h_{j+1,j}.  The Hessenberg matrix, its Givens rotations and the
 * back-substitution (at most 65 x 64 doubles) are on the host.  res_hist (host, >= maxiter entries): res_hist[it] =
 * |g_{j+1}|, the residual norm of the least-squares problem after iteration it; the loop stops when it is
 * < tol ||b||, at maxiter iterations, or when it is not finite (x then keeps the value of the last finished restart
 * cycle).  x += Z y at the end of every restart cycle and at the stop; every restart cycle starts from the explicit
 * residual b - A x.  ||r|| < tol ||b|| or ||r|| == 0 at entry: *n_iters = 0, x untouched.  ||w|| == 0 (the Krylov
 * space is exhausted): the entry is recorded, the cycle is finished and the loop stops; nothing is divided by it.
 * Small restart lengths can stagnate where a long one converges (restart 1 and 2 do on unsymmetric cycles of the
 * agglomerated DG hierarchy).
 * Work space: (2 restart + 2) N doubles on the context (V: restart + 1 vectors, Z: restart, and w) -- restart 30 at
 * 2^24 fine elements of p = 3 (N = 6.7e7) is 33 GB -- kept between calls of the same size, released when another size
 * is asked for and at aggmg_destroy.  When it cannot be allocated: AGGMG_ERR_HIP, the message names the bytes and the
 * restart length.  AGGMG_ERR_ARGUMENT, before anything is enqueued: NULL, restart outside
 * 1 .. AGGMG_FGMRES_MAX_RESTART, maxiter < 0, negative sweep counts, x_inout == b, a hierarchy created with
 * AGGMG_COARSE_EXTERNAL. */
#define AGGMG_FGMRES_MAX_RESTART 64
int aggmg_fgmres_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, double* x_inout, int restart, int maxiter, double tol,
                     int nPre, int nPost, double alpha, double* res_hist, int* n_iters);
/* The same two passes over ncols independent bases at once (what aggmg_fgmres_multi_dev runs per iteration).  Basis
 * vector i of column c is V + i * bstride + c * cstride (basis index outer, column inner; bstride, cstride >= n), its
 * vector is W + c * ldw (ldw >= n); 1 <= nvec <= AGGMG_FGMRES_MAX_RESTART + 1, ncols >= 1.  Both synchronous.
 * aggmg_multi_dot_cols_dev: out_host[c * nvec + i] = V_i[:, c] . W[:, c], one pass over W per group of 8 vectors for all
 * columns, one launch that finishes all ncols * nvec sums; entry (c, i) is bit for bit aggmg_multi_dot_dev's entry i on
 * column c alone, hence aggmg_dot_dev's.
 * aggmg_multi_axpy_norm_cols_dev: W[r, c] <- fma(coef_host[c * nvec + nvec-1], V_{nvec-1}[r, c], ... fma(coef_host[c * nvec],
 * V_0[r, c], W[r, c])) for r < n (ascending i, in place; rows >= n and other columns are not touched); norm_out_host
 * (ncols entries, may be NULL) receives ||W[:, c]||_2 of the stored columns: the bits aggmg_multi_axpy_norm_dev stores
 * and returns on column c alone.
 * AGGMG_ERR_ARGUMENT: NULL, n < 0, nvec outside 1 .. 65, ncols < 1, a stride or ldw < n, W overlapping V. */
int aggmg_multi_dot_cols_dev(aggmg_ctx* ctx, const double* V, int64_t n, int64_t nvec, int64_t ncols, int64_t bstride,
                             int64_t cstride, const double* W, int64_t ldw, double* out_host);
int aggmg_multi_axpy_norm_cols_dev(aggmg_ctx* ctx, const double* V, int64_t n, int64_t nvec, int64_t ncols, int64_t bstride,
                                   int64_t cstride, const double* coef_host, double* W_inout, int64_t ldw,
                                   double* norm_out_host);
/* aggmg_fgmres_dev on K right-hand sides: K recurrences in lockstep, each with its own Hessenberg matrix and rotations
 * on the host.  B, X_inout: device, column-major, leading dimension ld >= N; X holds the initial guesses and the
 * results.  Per iteration j of a restart cycle, on the kact columns still active: Z_j = M^-1 V_j by one K-column cycle
 * from zero guesses (aggmg_vcycle_multi_dev), W = -A Z_j by the K-column residual, the dots and the update + norms of all
 * columns in one launch sequence (aggmg_multi_dot_cols_dev's / aggmg_multi_axpy_norm_cols_dev's passes), ONE read-back of
 * all columns' h_0..j and ||w||, v_{j+1} = w / ||w|| for all columns in one launch.  Column j's iterate, n_iters[j] and
 * res_hist[j * maxiter + i] are bit for bit aggmg_fgmres_dev's on column j with the same arguments: the column stops when
 * res < tol ||b_j|| (its own ||b_j||), at maxiter iterations (the last restart cycle is cut, as there), when ||w|| == 0
 * (nothing is divided by it) or when a history entry is not finite (x_j then keeps the value of its last finished
 * restart cycle); ||r_j|| == 0 or < tol ||b_j|| at the start of a restart cycle stops it -- at entry: n_iters[j] = 0 and
 * x_j untouched.  All active columns share the position in the restart cycle, and a column's iteration counter is the
 * common one until it leaves.  A column that has stopped is final: its x_j += Z y is applied at once, it leaves the
 * active set, the last active column's state takes its place, and it costs no further work; *work_cols (may be NULL)
 * returns the column-V-cycles actually run (= the sum of n_iters).  res_hist: host, ncols * maxiter entries; n_iters:
 * host, ncols entries.  Hierarchies the K-column cycle or residual does not cover (aggmg_hier_multi_info: fused = 0;
 * CG chain operators) run their column-by-column forms under the same contract.
 * Work space: (2 restart + 2) N ncols doubles on the context -- V[j][column slot][N], Z[j][slot][N], W[slot][N] -- kept
 * between calls of the same size, released when another size is asked for (by this solver or by aggmg_fgmres_dev, which
 * shares it) and at aggmg_destroy; per-column scalars and partial sums (540 kB per column) grow with the largest ncols
 * seen.  When the work space cannot be allocated: AGGMG_ERR_HIP, the message names the bytes, restart and ncols.
 * AGGMG_ERR_ARGUMENT, before anything is enqueued: NULL, ncols < 1, ld < N, restart outside
 * 1 .. AGGMG_FGMRES_MAX_RESTART, maxiter < 0, negative sweep counts, X overlapping B, a hierarchy created with
 * AGGMG_COARSE_EXTERNAL. */
int aggmg_fgmres_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* B, double* X_inout, int64_t ncols, int64_t ld,
                           int restart, int maxiter, double tol, int nPre, int nPost, double alpha, double* res_hist,
                           int* n_iters, int64_t* work_cols);
/* ---- K right-hand sides through the outer loops (EXTENSION: the reference's solvers take vectors,
 * src/solvers.jl:116-139).  All matrices: device, column-major, leading dimension ld >= N (>= n). ---- */
/* out_host[j] = X[:, j] . Y[:, j] / ||X[:, j]||_2, j < ncols, each in one pass over the matrices: bit for bit
 * aggmg_dot_dev / aggmg_norm2_dev on column j.  Synchronous (the scalars come back in one copy). */
int aggmg_dot_cols_dev(aggmg_ctx* ctx, const double* X, const double* Y, int64_t n, int64_t ncols, int64_t ld,
                       double* out_host);
int aggmg_norm2_cols_dev(aggmg_ctx* ctx, const double* X, int64_t n, int64_t ncols, int64_t ld, double* out_host);
/* aggmg_pcg_dev on K right-hand sides: K conjugate-gradient recurrences in lockstep, each with its own scalars (on
 * the device), preconditioned by one K-column cycle from zero guesses (aggmg_vcycle_multi_dev), q = -A p from the
 * K-column residual.  X holds the initial guesses and the results.  Column j's iterate, n_iters[j] and
 * res_hist[j * maxiter + i] are bit for bit aggmg_pcg_dev's on column j (column j stops when ||r_j|| < tol ||b_j||).
 * A column that has met its tolerance leaves the active set and costs no further work; *work_cols (may be NULL)
 * returns the column-V-cycles actually run.  res_hist: host, ncols * maxiter entries; n_iters: host, ncols entries.
 * Hierarchies the K-column cycle does not cover (aggmg_hier_multi_info: fused = 0) run its column-by-column form
 * under the same contract.  Work space (4 N x ncols matrices) lives on the context; a repeated call allocates
 * nothing.  AGGMG_ERR_ARGUMENT: NULL, ncols < 1, ld < N, X overlapping B, nPre != nPost, negative counts, a hierarchy
 * created with AGGMG_COARSE_EXTERNAL. */
int aggmg_pcg_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* B, double* X_inout, int64_t ncols, int64_t ld,
                        int maxiter, double tol, int nPre, int nPost, double alpha, double* res_hist, int* n_iters,
                        int64_t* work_cols);
/* ---- conjugate gradients around the element-partitioned cycle (EXTENSION: aggmg_pcg_dev's recurrence with every
 * global scalar a rank-ordered sum of the ranks' owned terms; the reference has neither a partition nor a Krylov loop).
 * A local vector holds a rank's owned rows and its ghost rows; the owned rows are `nranges` <= 4 index ranges
 * [lo[g], hi[g]) of the local numbering (host arrays).  All three run on the context's stream; the two that return a
 * scalar synchronise it, as aggmg_dot_dev does.  Fixed slices, strides and summation trees, no atomics: the same bits
 * from run to run (for vectors at the same offsets from a 16-byte boundary).  AGGMG_ERR_ARGUMENT: NULL, more than 4
 * ranges, a range with lo < 0 or hi < lo, two non-empty ranges that overlap, aliased vectors; hi > n where the call
 * takes n. ---- */
/* *out = sum over the ranges of x_i y_i: one partial-sum launch over all ranges, one final launch.  The call takes no
 * vector length, so hi[g] is NOT checked against the end of x and y: the caller guarantees every range lies inside
 * both. */
int aggmg_owned_dot_dev(aggmg_ctx* ctx, const double* x, const double* y, int nranges, const int64_t* lo,
                        const int64_t* hi, double* out);
/* x += a p, r += a q on the n rows of the local vectors, and in the same pass *rr_out = sum over the ranges of the new
 * r_i^2.  With q = -A p (aggmg_residual_dev with a zero right-hand side) and a = rz / (-(p.q)) this is the step of
 * aggmg_pcg_dev; a arrives by value because the global scalars are on the host after the sum over the ranks. */
int aggmg_pcg_xr_owned_dev(aggmg_ctx* ctx, int64_t n, double* x, double* r, const double* p, const double* q, double a,
                           int nranges, const int64_t* lo, const int64_t* hi, double* rr_out);
/* p = z + beta p on n rows.  Asynchronous. */
int aggmg_pcg_p_dev(aggmg_ctx* ctx, int64_t n, double* p, const double* z, double beta);
/* ---- flexible GMRES around the element-partitioned cycle (EXTENSION: aggmg_fgmres_dev's recurrence with every global
 * scalar a rank-ordered sum of the ranks' owned terms -- the Krylov loop for partitioned cycles that are not symmetric:
 * hybrid element-patch levels, nPre != nPost).  The passes of its orthogonalisation over a device basis V (vector i at
 * V + i * ld, 1 <= nvec <= AGGMG_FGMRES_MAX_RESTART + 1) and a local device vector w, with the owned rows given as for
 * aggmg_owned_dot_dev.  Fixed slices, strides and summation trees, no atomics: the same bits from run to run, and the
 * same bits whether or not the basis vectors share w's offset from a 16-byte boundary (an odd ld walks the same pairs
 * with 8-byte accesses).  AGGMG_ERR_ARGUMENT, before anything is enqueued: NULL, nvec outside 1 .. 65, ld smaller than
 * the rows read, more than 4 ranges, a bad range or overlapping ranges, w overlapping V. ---- */
/* out_host[i] = sum over the ranges of V_i[r] w[r], i < nvec: one pass over w per group of 8 vectors, one launch that
 * finishes all sums, one read-back; synchronous.  Entry i is bit for bit aggmg_owned_dot_dev(w, V_i) on the same ranges
 * (w first: its address fixes the pair grid).  As there, the call takes no vector length: every range must lie inside w
 * and every V_i; ld must reach the end of the last range. */
int aggmg_owned_multi_dot_dev(aggmg_ctx* ctx, const double* V, int64_t nvec, int64_t ld, const double* w, int nranges,
                              const int64_t* lo, const int64_t* hi, double* out_host);
/* w[r] <- fma(c[nvec-1], V_{nvec-1}[r], ... fma(c[0], V_0[r], w[r])) on all n local rows (ascending i, in place, groups
 * of 8, one pass over w per group; rows >= n are not touched; ld >= n): the values aggmg_multi_axpy_norm_dev stores.
 * *sumsq_out_host (may be NULL) receives the sum over the ranges of the squares of the stored values, formed by the
 * pass that stores them -- NOT its root: the caller adds the ranks' sums first.  Synchronous with it; without it the
 * call only enqueues (coef_host has been read when it returns). */
int aggmg_owned_multi_axpy_norm_dev(aggmg_ctx* ctx, int64_t n, const double* V, int64_t nvec, int64_t ld, const double* coef_host,
                                    double* w_inout, int nranges, const int64_t* lo, const int64_t* hi, double* sumsq_out_host);
/* v[r] = w[r] / s on n rows: a division, not a multiplication by the reciprocal (v_{j+1} = w / h_{j+1,j} as
 * aggmg_fgmres_dev forms it); s arrives by value because the global norm is on the host after the sum over the ranks.
 * v may be w itself.  Asynchronous.  AGGMG_ERR_ARGUMENT: NULL, n < 0, s == 0 or not finite, v overlapping w partly. */
int aggmg_div_scalar_dev(aggmg_ctx* ctx, int64_t n, const double* w, double s, double* v);
/* aggmg_multigrid_dev on K right-hand sides: check_every K-column cycles, then the K-column residual and the column
 * norms, column j stopping when ||b_j - A x_j|| < tol ||b_j||.  Column j of X and n_cycles[j] / n_checks[j] are
 * bit for bit aggmg_multigrid_dev's on column j; res_hist[j * n_checks_max + i] (and err_hist, ||x_j - U_exact[:, j]||,
 * when U_exact and err_hist are given -- both or neither) are bit for bit those of its AGGMG_OPT_MG_CHECKPOINT = 0
 * form, n_checks_max = ceil(maxiter / check_every).  maxiter == 0: X = 0, no checks.  Finished columns leave the
 * active set; *work_cols (may be NULL): column-V-cycles actually run.  Work space (4 N x ncols matrices) on the
 * context.  AGGMG_ERR_ARGUMENT: NULL, ncols < 1, ld < N, check_every < 1, X overlapping X0, B or U_exact, U_exact
 * without err_hist or the reverse, negative counts, a hierarchy created with AGGMG_COARSE_EXTERNAL. */
int aggmg_multigrid_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* X0, const double* B, int64_t ncols, int64_t ld,
                              int maxiter, double tol, int check_every, int nPre, int nPost, double alpha, double* X,
                              double* res_hist, int* n_cycles, int* n_checks, const double* U_exact, double* err_hist,
                              int64_t* work_cols);

/* ---- measurement ---------------------------------------------------------------------------- */
/* HIP-event timing of kernel launches on the context stream, by tag = kind * 16 + level
 * (level < 16; level 0 for the stand-alone fused ops).  While enabled every launch is bracketed
 * by two events; aggmg_profile_collect synchronises and returns per-tag total ms and counts
 * (arrays of AGGMG_PROFILE_NTAGS), then resets. */
#define AGGMG_PROFILE_NTAGS 256
#define AGGMG_KIND_FUSED_DOWN 0 /* [u=0|x0] -> nPre sweeps -> residual -> restriction */
#define AGGMG_KIND_FUSED_UP 1   /* prolong-add -> nPost sweeps */
#define AGGMG_KIND_SMOOTH 2     /* structured multi-sweep smoother kernel */
#define AGGMG_KIND_RESIDUAL 3
#define AGGMG_KIND_RESTRICT 4
#define AGGMG_KIND_PROLONG 5
#define AGGMG_KIND_JACOBI 6      /* generic CSR fused point-Jacobi sweep */
#define AGGMG_KIND_BLOCK_APPLY 7 /* generic gather block apply */
#define AGGMG_KIND_COARSE 8      /* device coarsest solve (all its launches) */
#define AGGMG_KIND_FUSED_MID 9   /* prolong-add -> nPost + nPre sweeps -> restriction (between cycles) */
/* aggmg_hier_launch_bytes only (no profile tag: the launches are timed as _FUSED_DOWN / _FUSED_UP): the two launches of
 * a replayed cycle (AGGMG_OPT_REPLAY_PRESMOOTH) */
#define AGGMG_KIND_REPLAY_DOWN 10 /* _FUSED_DOWN without the store of the pre-smoothed iterate */
#define AGGMG_KIND_REPLAY_UP 11   /* [u=0|x0] -> nPre sweeps -> prolong-add -> nPost sweeps */
/* on: 0 = off, 1 = every launch, 2 = only the fine-level fused-down launch (the dominant kernel:
 * one event pair per cycle, so that timing it does not disturb the cycle being timed -- an event pair
 * costs ~7 us of stream time on MI355X). */
int aggmg_profile_enable(aggmg_ctx* ctx, int on);
int aggmg_profile_collect(aggmg_ctx* ctx, double* total_ms, int64_t* counts);
/* Compulsory HBM bytes of one launch: the sizes of the arrays the launch has to read and to write, each counted
 * once, in the format the level stores them (index-free block rows, packed symmetric inverses, transfer rows) --
 * no halo re-reads, no cache effects, no CSR model.  bytes / launch duration / 8 TB/s is the launch's roofline
 * fraction (<= 1 by construction; measurement aid, no reference counterpart).
 * aggmg_hier_launch_bytes: the fused launch of `level` (not the coarsest) that aggmg_vcycle_dev enqueues, kind =
 * AGGMG_KIND_FUSED_DOWN (src/solvers.jl:28-37), _UP (:41-47) or _MID (both, between the cycles of aggmg_vcycles_dev);
 * has_x0: the descent reads an initial guess (level 0).  AGGMG_ERR_UNSUPPORTED on a level that runs the generic kernels.
 * _FUSED_DOWN and _FUSED_UP describe the launches that STORE the pre-smoothed iterate and read it back; a cycle that
 * replays its pre-smoothing (AGGMG_OPT_REPLAY_PRESMOOTH, the default of aggmg_vcycle_dev where it applies) runs
 * AGGMG_KIND_REPLAY_DOWN -- the same without that store -- and AGGMG_KIND_REPLAY_UP, which reads the first iterate in
 * the stored one's place (has_x0 = 0: no iterate at all).
 * aggmg_smoother_launch_bytes: what = 0 one launch of aggmg_smooth_dev (any number of sweeps that fit one launch),
 * what = 1 aggmg_residual_dev (sm may be NULL). */
int aggmg_hier_launch_bytes(aggmg_ctx* ctx, const aggmg_hier* h, int level, int kind, int has_x0, int64_t* read_bytes,
                            int64_t* write_bytes);
/* compulsory bytes of one K-column fused launch (aggmg_vcycle_multi_dev, kind = AGGMG_KIND_FUSED_DOWN / _UP): the
 * operator's arrays once, the vectors' once per column -- ncols = 1 gives aggmg_hier_launch_bytes' figures */
int aggmg_hier_multi_launch_bytes(aggmg_ctx* ctx, const aggmg_hier* h, int level, int kind, int has_x0, int64_t ncols,
                                  int64_t* read_bytes, int64_t* write_bytes);
int aggmg_smoother_launch_bytes(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, int what, int64_t* read_bytes,
                                int64_t* write_bytes);
/* compulsory bytes of one K-column residual launch (aggmg_residual_multi_dev, EXTENSION): the operator's entry arrays
 * once, X (and B when has_b) once per column, R once per column.  AGGMG_ERR_UNSUPPORTED on an operator that runs
 * column by column. */
int aggmg_residual_multi_launch_bytes(aggmg_ctx* ctx, aggmg_op* A, int64_t ncols, int has_b, int64_t* read_bytes,
                                      int64_t* write_bytes);

/* Library / build identification ("aggmg_hip gfx950 ..."). */
const char* aggmg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* AGGMG_HIP_H */
