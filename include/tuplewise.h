/*
 * tuplewise.h — C ABI of libtuplewise.so, the MI355X (gfx950) implementation of the
 * tuplewise hot path of "Trade-offs in Large Scale Distributed Tuplewise Estimation and
 * Learning" (reference: RobinVogel/Trade-offs-in-Distributed-Tuplewise-Estimation-and-Learning).
 *
 * The reference is pure Python/NumPy; its boundary is the `f_block(X_block, Z_block)`
 * protocol consumed by UN / UN_split (learning-experiment/compute_stats.py:44-92) and the
 * estimator functions that produce block values.  Each entry point below replaces the
 * per-shard NumPy body of one of those functions for ALL shards in one launch; the Python
 * package (tuplewise.compute_stats / tuplewise.estimation) keeps the reference names and
 * calls these through ctypes.
 *
 * Conventions
 *   - every pointer argument named d_* is DEVICE memory (hipMalloc / torch.cuda); everything
 *     else is a host scalar.  No entry point allocates, copies to/from the host, or
 *     synchronises: all work is enqueued on `stream` (a hipStream_t, NULL = default stream),
 *     so calls are graph-capturable.
 *   - shards are described by offset arrays: shard s owns elements [off[s], off[s+1]) of the
 *     concatenated input; n_shards+1 int64 entries, device memory.
 *   - dtype codes: TW_F64 (double), TW_I64 (int64).  Both sides of a call share one dtype
 *     (the Python layer applies NumPy's promotion rules first).
 *   - return value: TW_OK (0) or an error code; tw_last_error() gives a thread-local message.
 *     TW_ERR_ARG maps to the reference's AssertionError/ValueError, TW_ERR_HIP to RuntimeError.
 */
#ifndef TUPLEWISE_H
#define TUPLEWISE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TW_OK 0
#define TW_ERR_ARG 1
#define TW_ERR_HIP 2

#define TW_F64 0
#define TW_I64 1

/* Pair predicates.  TW_PRED_GT is the reference AUC kernel 1{x > z}
 * (estimation-experiment/main.py:31; compute_stats.py:19 `X - Z > 0`, identical for IEEE
 * doubles).  TW_PRED_HALF is the opt-in "+0.5 on ties" mode asked for by BASELINE.json: the
 * counter then holds half-units 2*#{x>z} + #{x==z} = #{x>z} + #{x>=z}.
 * TW_PRED_SUBGT is `(x - z) > 0` with int64 wrap-around, the literal cs.Un AUC body for int64
 * inputs (compute_stats.py:19, :30); for doubles it equals TW_PRED_GT. */
#define TW_PRED_GT 0
#define TW_PRED_HALF 1
#define TW_PRED_SUBGT 2

/* Float pair kernels of cs.Un / cs.UB_indices (compute_stats.py:15-18, :27-29) and the
 * hinge surrogate conv_AUC (compute_stats.py:129-135). */
#define TW_KERN_PROD 0  /* x * z                 */
#define TW_KERN_GINI 1  /* |x - z|               */
#define TW_KERN_HINGE 2 /* max(z - x + margin, 0) */
#define TW_KERN_LOGISTIC 3 /* log(1 + exp(z - x + margin)): extension, SURVEY.md §8 row L3 */

/* Pairwise losses of the gradient kernels.  TW_LOSS_HINGE is grad_inc_block's
 * (compute_stats.py:146-162).  TW_LOSS_LOGISTIC is the pairwise-logistic loss BASELINE.json
 * names, absent from the reference (parity pinned against
 * oracle/oracle.py only): softplus(S), S = diff . w + margin, pair weight sigma(S). */
#define TW_LOSS_HINGE 0
#define TW_LOSS_LOGISTIC 1

const char* tw_last_error(void);
int tw_version(void);
/* number of visible HIP devices (0 when no GPU); does not create a context on failure */
int tw_device_count(int* out_count);

/* ---- Row A1/A2/A6/A7: complete two-sample count, all shards in one launch -------------
 * Replaces est.Un (estimation-experiment/main.py:29-31) and cs.Un(kernel="AUC")
 * (compute_stats.py:10-19) as the f_block of UN (main.py:33-69, compute_stats.py:56-92).
 * d_out[s] (uint64) = #{(i,j): pred(x_i, z_j)} over shard s (half-units for TW_PRED_HALF).
 * max_nx / max_nz: the largest shard sizes (host-known; they size the grid). */
int tw_count_pairs(const void* d_x, const int64_t* d_x_off, const void* d_z,
                   const int64_t* d_z_off, int32_t n_shards, int64_t max_nx, int64_t max_nz,
                   int32_t dtype, int32_t pred, uint64_t* d_out, void* stream);

/* One step of est.UnNT's loop (estimation-experiment/main.py:76-79) in ONE launch: the counts
 * of the current partition exactly as tw_count_pairs — except that d_out must already be zero
 * (the kernel accumulates into it) — and, on spare leading blocks of the same grid, the NEXT
 * repartition: d_x_next = the n_x scores of d_x permuted with key_x, d_z_next likewise (as
 * tw_permute_pair), and d_out_next[0 .. n_next_shards) zeroed for the next step.
 * d_x_next == NULL: count only (d_out_next, if given, is zeroed by a memset). */
int tw_count_pairs_step(const void* d_x, const int64_t* d_x_off, const void* d_z,
                        const int64_t* d_z_off, int32_t n_shards, int64_t max_nx, int64_t max_nz,
                        int32_t dtype, int32_t pred, uint64_t* d_out, int64_t n_x, void* d_x_next,
                        uint64_t key_x, int64_t n_z, void* d_z_next, uint64_t key_z,
                        uint64_t* d_out_next, int32_t n_next_shards, void* stream);

/* Tuning hook for tw_count_pairs_step: number of spare blocks (0 = automatic), their
 * placement (tail = 1, the default: the last blocks of the grid; tail = 0: one group of 8
 * every `every` blocks, 0 = automatic spacing, 8 = the leading blocks).  Process-global;
 * results do not depend on it. */
int tw_count_step_set_plan(int32_t blocks, int32_t every, int32_t tail);

/* Tuning hook: 1 (default) counts part of each lane's x-values on the scalar unit (double
 * inputs, one-bit predicates; csrc/count.hip), 0 = VALU-only accumulation.  Process-global;
 * results do not depend on it. */
int tw_count_set_scalar_mix(int32_t on);

/* Tuning hook for tw_count_pairs' launch plan: R x-values per lane (1, 2, 4, 8; 0 = automatic)
 * and z-chunk length per block (0 = automatic).  Process-global; results do not depend on it. */
int tw_count_set_plan(int32_t R, int64_t z_chunk);

/* ---- A1/A6/A7 on rank images (round 3, csrc/rankimage.hip): the all-pairs count of
 * est.UnN / UnNT (estimation-experiment/main.py:29-31, :72-79) on packed f32 images.
 * tw_rank_images gives every score an 8-B record {low word: f32 image, high word: its index in
 * d_x / d_z}: image g(v) = #{z in d_z : z < v} (x: g, z: -g; a NaN x: -2^25), so that for any
 * pair x > z <=> x_image + z_image >= 1, NaN and -0 == +0 included (strict predicate, float64
 * or int64 scores; int64 SUBGT / half ties stay on tw_count_pairs).  One bucketed ranking of
 * X u Z per call (sampled splitters, per-bucket LDS sorts of the z keys); needs n_z < 2^24
 * (tw_rank_images_work_bytes returns -1 otherwise).
 * d_work: device scratch of tw_rank_images_work_bytes(n_x, n_z) bytes. */
int64_t tw_rank_images_work_bytes(int64_t n_x, int64_t n_z);
int tw_rank_images(const void* d_x, int64_t n_x, const void* d_z, int64_t n_z, int32_t dtype,
                   void* d_work, int64_t work_bytes, uint64_t* d_x_rec, uint64_t* d_z_rec,
                   void* stream);
/* tw_count_pairs_step on records: counts every shard of the current partition of d_x_rec /
 * d_z_rec into d_out (already zero) — per pair one packed clamp-add and one packed add — and,
 * when d_x_next is given, permutes both record arrays for the next step with the keyed Feistel
 * bijection (as tw_count_pairs_step permutes scores) and zeroes d_out_next, in the same launch.
 * Counts are identical to tw_count_pairs(..., TW_PRED_GT) on the scores the records index. */
int tw_count_pairs_rank_step(const uint64_t* d_x_rec, const int64_t* d_x_off,
                             const uint64_t* d_z_rec, const int64_t* d_z_off, int32_t n_shards,
                             int64_t max_nx, int64_t max_nz, uint64_t* d_out, int64_t n_x,
                             uint64_t* d_x_next, uint64_t key_x, int64_t n_z, uint64_t* d_z_next,
                             uint64_t key_z, uint64_t* d_out_next, int32_t n_next_shards,
                             void* stream);
/* The scores in record order: d_out[p] = d_in[d_rec[p] >> 32] (8-B values; in != out). */
int tw_gather_records(const void* d_in, const uint64_t* d_rec, int64_t n, void* d_out,
                      void* stream);
/* Tuning hook for tw_count_pairs_rank_step: x-images per lane R (8 or 16; 0 = automatic) and
 * z-chunk length (0 = automatic).  Process-global; results do not depend on it. */
int tw_count_rank_set_plan(int32_t R, int64_t z_chunk);
/* Tuning hook for tw_count_pairs_rank_step's fused next repartition: its spare blocks are the
 * last blocks of the grid (front = 0, the default) or the first (front = 1).  Process-global;
 * results do not depend on it. */
int tw_count_rank_set_next(int32_t front);
/* Tuning hook for tw_rank_images / tw_rank_images_query: sampled z keys for the splitters (512,
 * 1024 or 2048) and z per thread in the bucket passes (4, 8 or 16).  Process-global; results
 * do not depend on it (the workspace size does: query it after setting). */
int tw_rank_set_plan(int32_t sample, int32_t per);
/* Tuning hook for small Z (n_z <= 2^18: the one-shot C2 counts): the ranking's sample size
 * (256, 512, 1024 or 2048 keys; default 256), the target z per interval bucket (512, 1024 or
 * 2048; default 2048) and z per thread in the bucket passes (4, 8 or 16; default 4). */
int tw_rank_set_small(int32_t sample, int32_t z_per_interval, int32_t per);
/* tw_rank_images over several ranks (and for half ties): the images are counted against the Z
 * of d_z_all (the all-gathered sample, n_z_all < 2^24) but written only for the n_x + n_z
 * elements of d_x / d_z (this rank's share; d_z may be d_z_all).  half (flags): bit 0 — each X
 * record's high word is h(x) = #{z in d_z_all : z <= x} as f32 bits (NaN x: -2^25) instead of
 * the index; bit 1 — compact images without indices, the bag layout of tw_count_pairs_chain
 * (d_x_rec: n_x f32, or n_x {g, h} f32 pairs with bit 0; d_z_rec: n_z f32).
 * d_work: tw_rank_images_work_bytes(n_x, n_z_all) bytes. */
int tw_rank_images_query(const void* d_z_all, int64_t n_z_all, const void* d_x, int64_t n_x,
                         const void* d_z, int64_t n_z, int32_t dtype, int32_t half,
                         void* d_work, int64_t work_bytes, uint64_t* d_x_rec, uint64_t* d_z_rec,
                         void* stream);

/* ---- A7 / (e) step chains (round 4, csrc/chain.hip): the repartition loop of est.UnNT
 * (estimation-experiment/main.py:76-79; each repartition = the keyed Feistel bijection of
 * tw_permute_pair with keys 2k / 2k+1) walked per element.  A rank holds n_x + n_z elements
 * whose global indices start at rank * n_x / rank * n_z in samples of world * n_x / world * n_z;
 * every rank's local layout is prop-SWOR shards of x_shard / z_shard positions (n_shards of
 * them, clamped at the array ends, then a tail in no shard).
 * tw_chain_emit walks `steps` (<= 32) repartitions (host arrays keys_x / keys_z of the Feistel
 * keys) for every element of d_x_rec / d_z_rec (rank-image records; half = 1: X records carry
 * {g, h}), its global position kept in d_x_pos / d_z_pos (u32; first = 1: start from the
 * element's global index).  d_send == NULL (one process, world == 1): for each step c the
 * images are appended to the bags d_x_bag [steps][n_x] (f32, or {g, h} f32 pairs when half) /
 * d_z_bag [steps][n_z] (f32), each shard's slot range holding exactly its images in an
 * arbitrary order; d_cursors: scratch of steps * 2 * (n_shards + 1) u32.  d_send given (the
 * exchange: world > 1, or a world-size-1 group forced through its collectives): records go to
 * d_send, per destination rank g a
 * chunk of steps buckets of (cap + 1) * W u64 words (W = 1 + half; word 0 of a bucket = its
 * count), each record {image word(s), local position (Z: n_x + position)}; a bucket past cap
 * sets *d_flag (the record is dropped). */
int tw_chain_emit(const uint64_t* d_x_rec, int64_t n_x, const uint64_t* d_z_rec, int64_t n_z,
                  int32_t half, uint32_t* d_x_pos, uint32_t* d_z_pos, int32_t first,
                  int32_t rank, int32_t world, const uint64_t* keys_x, const uint64_t* keys_z,
                  int32_t steps, int64_t x_shard, int64_t z_shard, int32_t n_shards,
                  void* d_x_bag, void* d_z_bag, uint32_t* d_cursors, uint64_t* d_send,
                  int64_t cap, int32_t* d_flag, void* stream);
/* tw_chain_emit with round tables: where both permutation domains are small
 * enough (world * n_x and world * n_z <= 2^22) the six Feistel round functions of every (step,
 * class) are tabulated once per call into d_work and each block looks its rounds up in LDS —
 * the same permutations bit for bit, without the rounds' multiplies.  d_work: caller-provided,
 * 16-B aligned, at least tw_chain_emit_work_bytes(steps, world * n_x, world * n_z) bytes (else
 * TW_ERR_ARG before any launch); written and read inside this one call on this one stream, so
 * calls on one stream may reuse it and calls on different streams need their own.  Larger
 * domains (work bytes 0) run tw_chain_emit's arithmetic rounds; tw_chain_emit itself always
 * does. */
int tw_chain_emit_ws(const uint64_t* d_x_rec, int64_t n_x, const uint64_t* d_z_rec, int64_t n_z,
                     int32_t half, uint32_t* d_x_pos, uint32_t* d_z_pos, int32_t first,
                     int32_t rank, int32_t world, const uint64_t* keys_x, const uint64_t* keys_z,
                     int32_t steps, int64_t x_shard, int64_t z_shard, int32_t n_shards,
                     void* d_x_bag, void* d_z_bag, uint32_t* d_cursors, uint64_t* d_send,
                     int64_t cap, int32_t* d_flag, void* d_work, int64_t work_bytes,
                     void* stream);
int64_t tw_chain_emit_work_bytes(int32_t steps, int64_t NX, int64_t NZ);
/* Tuning hook for tw_chain_emit_ws's round tables: 0 automatic (one process with strict ties,
 * 8 elements per thread, one step per round, domains up to 2^20: where the sweep of DESIGN
 * §4.1c found them faster), 1 off (the arithmetic rounds), 2 on wherever a table fits; -1
 * reports.  Returns the previous setting; any other value is TW_ERR_ARG (tw_last_error names
 * it) and changes nothing.  Process-global; results do not depend on it. */
int32_t tw_chain_set_emit_tables(int32_t mode);
/* 1 where the tw_chain_emit_ws launch with these arguments (exchange: d_send given) looks its
 * rounds up under the current settings (this hook and tw_chain_set_emit), 0 where it runs the
 * arithmetic rounds: the launch's own decision.  Under the automatic rule half ties, the
 * exchange and more than 512 buckets run the arithmetic rounds. */
int32_t tw_chain_emit_tables_of(int64_t n_x, int64_t n_z, int32_t world, int32_t half,
                                int32_t exchange, int32_t n_shards);
/* The receiving side of tw_chain_emit's buckets after an equal-split all-to-all (d_recv: world
 * chunks in source order): every record appended to the bag region of its (step, side, shard)
 * — shard b of a side holds positions [min(b k, n), min((b+1) k, n)), k = x_shard / z_shard,
 * b = n_shards the tail — in runs reserved on d_cursors (steps x 2 (n_shards + 1) u32, zeroed
 * here); a bag holds its shard's multiset, in no particular order (what the counts read).  A
 * count past cap sets *d_flag. */
int tw_chain_unpack(const uint64_t* d_recv, int32_t world, int32_t steps, int64_t cap,
                    int32_t half, int64_t n_x, int64_t n_z, int64_t x_shard, int64_t z_shard,
                    int32_t n_shards, void* d_x_bag, void* d_z_bag, uint32_t* d_cursors,
                    int32_t* d_flag, void* stream);
/* The all-pairs counts of `steps` x n_shards bags in ONE launch: bag (c, s) = x images
 * [c * x_stride + d_x_off[s], c * x_stride + d_x_off[s + 1]) against z images likewise;
 * d_out[c * n_shards + s] (zeroed here) = #{x > z} (half = 1: 2 #{x > z} + #{x == z}, the
 * tw_count_pairs TW_PRED_HALF units).  Identical to tw_count_pairs on the scores. */
int tw_count_pairs_chain(const void* d_x_bag, const int64_t* d_x_off, int64_t x_stride,
                         const void* d_z_bag, const int64_t* d_z_off, int64_t z_stride,
                         int32_t n_shards, int32_t steps, int64_t max_nx, int64_t max_nz,
                         int32_t half, uint64_t* d_out, void* stream);
/* tw_count_pairs_chain with the caller's promise that every x and z image is an integer in
 * [0, image_bound] (x images also: the -2^25 "never" image of a NaN score).  With the strict
 * predicate (half = 0) and image_bound < 2^24 the count runs bit-sliced (32 pairs
 * per lane and instruction) on bit planes built ONCE per bag: a pre-pass
 * (k_chain_planes) writes the planes of every bag's x groups (and of its z groups, where the x
 * remainder is counted with the roles swapped) into d_work, and the count
 * (k_count_chain_planes or its class-run form) follows on the same stream inside this call.
 * half = 1, a bound of 2^24 or more, and bags much smaller than a plane tile (chainplan.h
 * chain_count_sliced) run tw_count_pairs_chain's packed kernel.  The counts are the same either
 * way.  d_work: at least tw_chain_planes_work_bytes(...) bytes (else TW_ERR_ARG before any
 * launch), written and read only inside the call — calls on different streams must not share
 * it. */
int tw_count_pairs_chain_planes(const void* d_x_bag, const int64_t* d_x_off, int64_t x_stride,
                                const void* d_z_bag, const int64_t* d_z_off, int64_t z_stride,
                                int32_t n_shards, int32_t steps, int64_t max_nx, int64_t max_nz,
                                int32_t half, int64_t image_bound, uint64_t* d_out,
                                void* stream, void* d_work, int64_t work_bytes);
/* Bytes of d_work for tw_count_pairs_chain_planes / tw_chain_unpack_count_planes on steps x
 * n_shards bags of at most max_nx x max_nz images (0 where the count runs packed): the planes
 * and the class-run form's regions (the class-ordered z images and the run
 * tables), sized for any plan and any class bits, so the tuning hooks do not change it. */
int64_t tw_chain_planes_work_bytes(int32_t n_shards, int32_t steps, int64_t max_nx,
                                   int64_t max_nz, int32_t half, int64_t image_bound);
/* The form of the class loop a count with nb planes and k class bits runs (DESIGN §4.1h,
 * §4.1i): 3 = the digit tables, where nb - k low planes fit them; 2 = masked planes and scalar
 * loads.  A query: there is no hook to set it. */
int32_t tw_count_chain_class_form(int32_t nb, int32_t k);
/* A/B control of the digit loop's items: an item walks a span of `runs`
 * consecutive run-table entries of its bag and keeps what depends on its x tile alone across
 * them.  runs >= 1 forces the span (clamped to each launch's table capacity; 1 is one item per
 * entry), 0 restores the automatic rule (chainclass.h class_span_auto), -1 only reports, any
 * other value changes nothing.  Returns the setting in force before the call.  Process-global;
 * same counts; the masked-plane loop (form 2) always runs one entry per item. */
int32_t tw_count_chain_class_span(int32_t runs);
/* A/B control of the digit loop's split: planes per digit.  4 runs the wide
 * digits — three tables of 16 (+ 1) entries, 4 VALU and 5 SALU per z image and group instead
 * of 5 and 7 — where nb - k = 12 and the four-digit loop anywhere else; 3 forces the four-digit
 * loop everywhere; 0 restores the automatic rule (chainclass.h kClassDigitsAuto: wide where it
 * fits); -1 only reports.  Returns the setting in force before the call (0, 3 or 4); any other
 * value changes nothing and returns TW_ERR_ARG.  Process-global; same counts, same workspace:
 * every launch re-encodes its z region for the loop it runs. */
int32_t tw_count_chain_class_digits(int32_t w);
/* The planes per digit a count with nb planes and k class bits runs under the current setting:
 * 4 where it runs the wide digits, 3 anywhere else (where the launch runs no digit loop — see
 * tw_count_chain_class_form — the setting has no effect). */
int32_t tw_count_chain_class_digits_of(int32_t nb, int32_t k);
/* A/B control of the class count's LDS-table form: where a launch would run the
 * wide digits, one block of 16 waves per (bag, x tile of two groups) tabulates the carries of
 * the low 8 planes in 128 KiB of LDS and its waves read them from there — 5 VALU per z image
 * instead of 8.  0: the automatic rule (chainclass.h class_lds_runs); 1: off, every launch is
 * the digit loops'; 2: on wherever the form fits (the wide digits would run, two groups per
 * tile, no swapped items in the plan); -1 only reports.  Returns the setting in force before
 * the call; any other value changes nothing and returns TW_ERR_ARG.  Process-global; same
 * counts, same workspace: every launch re-encodes its z region for the loop it runs.
 * tw_count_chain_class_span has no effect on a launch of this form. */
int32_t tw_count_chain_class_lds(int32_t mode);
/* 1 if a strict tw_count_pairs_chain_planes launch with these arguments runs the LDS-table form
 * under the current settings, 0 if it runs any other. */
int32_t tw_count_chain_class_lds_of(int32_t n_shards, int32_t steps, int64_t max_nx,
                                    int64_t max_nz, int64_t image_bound);
/* A/B control of how the class-run form's pre-passes are launched.  0 (automatic)
 * and 2: one launch (k_chain_prepass) builds the planes, sorts every bag's z images into class
 * runs — in registers, one pass over global memory, for bags of up to 16384 z images — and
 * zeroes the counts; 1: the separate launches (the zeroing, k_chain_planes, k_chain_zclasses);
 * -1 only reports.  Returns the setting in force before the call; any other value changes
 * nothing and returns TW_ERR_ARG.  Process-global; same counts, same workspace regions: every
 * launch rewrites its regions before its count, so the forms may alternate on one workspace. */
int32_t tw_count_chain_prepass(int32_t mode);
/* The form a strict tw_count_pairs_chain_planes launch with these arguments runs under the
 * current settings: 0 no pre-pass (the packed kernel), 1 separate launches (also every launch
 * without class bits), 2 fused with every bag sorted in registers, 3 fused with the two-pass
 * streaming loop for the bags of more than 16384 z images. */
int32_t tw_count_chain_prepass_of(int32_t n_shards, int32_t steps, int64_t max_nx,
                                  int64_t max_nz, int64_t image_bound);
/* The same counts as tw_count_pairs_chain in O(n + m) per bag (algo="sorted", SURVEY row f4;
 * estimation-experiment/main.py:29-31's integer): each bag's z images (integers in
 * [0, z_total], z_total = the Z count the images were ranked against) counting-sorted into
 * <= 16384 LDS buckets, every x's g(x) (and h(x) with half) answered by the bucket prefix and a
 * scan of its own bucket.  Bags of <= 16384 z (max_nz); d_out[c * n_shards + s] written, not
 * accumulated. */
int tw_count_pairs_chain_bucket(const void* d_x_bag, const int64_t* d_x_off, int64_t x_stride,
                                const void* d_z_bag, const int64_t* d_z_off, int64_t z_stride,
                                int32_t n_shards, int32_t steps, int64_t max_nz,
                                int64_t z_total, int32_t half, uint64_t* d_out, void* stream);
/* Tuning hook for tw_chain_emit: elements per thread (2, 4 or 8) and steps per reservation
 * round (1 or 16 / elements per thread); 0 = automatic.  Process-global; results do not depend
 * on it (the order inside a bag does). */
int tw_chain_set_emit(int32_t epr, int32_t steps_per_round);
/* Tuning hook for tw_count_pairs_chain and its _bound / _planes forms: R = 8 or 16 x-images per
 * lane forces the packed kernel, R = 2, 3 or 4 plane groups per lane (3: the _planes form; the
 * _bound form takes it as 4) the bit-sliced one (where
 * the call allows it: a bound below 2^24, strict predicate), 0 = automatic; z-chunk length
 * for either kernel (0 = automatic).  Process-global; results do not depend on it. */
int tw_count_chain_set_plan(int32_t R, int64_t z_chunk);
/* A/B hook for tw_count_pairs_chain_planes: 0 counts every x remainder as a padded plane group
 * (no swapped items), 2 swaps wherever chainplan.h's per-bag rule allows, 1 (default) does so
 * in launches large enough to gain from it and, under class runs, only where the swapped
 * remainder also costs fewer instructions than a padded group (chainclass.h class_swap_mode,
 * DESIGN §4.1h).  Process-global; same counts. */
int tw_count_chain_set_swap(int32_t swap);
/* A/B hook for tw_count_pairs_chain_planes' class-run form: the z images of a
 * bag grouped by their top k bits once per launch (k_chain_zclasses) and counted run by run of
 * one class (k_count_chain_classes), the class's top-field compare hoisted out of the per-z
 * loop.  k = -1 (default) chooses by chainclass.h's rule, 0 turns classes off
 * (k_count_chain_planes), 1 <= k <= 8 forces k class bits; anything else is TW_ERR_ARG.
 * Process-global; same counts. */
int tw_count_chain_set_class_bits(int32_t k);
/* The scores in their final order after the chains (one process): d_x_out[d_x_pos[e]] =
 * d_x[e] (8-B values), likewise for Z. */
int tw_chain_scatter(const void* d_x, const uint32_t* d_x_pos, int64_t n_x, const void* d_z,
                     const uint32_t* d_z_pos, int64_t n_z, void* d_x_out, void* d_z_out,
                     void* stream);

/* ---- f4: the same counts in O((n+m) log m): sort each z-chunk (<= 16384 keys) in LDS as
 * order-preserving u64 keys, then binary-search every x (csrc/rankcount.hip).  Bit-identical
 * to tw_count_pairs for TW_PRED_GT and TW_PRED_HALF (not SUBGT).  d_work: device scratch of
 * tw_count_pairs_sorted_work_bytes(n_shards, max_nz) bytes. */
int64_t tw_count_pairs_sorted_work_bytes(int32_t n_shards, int64_t max_nz);
/* Tuning hook: largest sorted chunk (power of two in [1024, 16384]; default 4096).
 * Process-global; results do not depend on it (the workspace size does). */
int tw_count_sorted_set_chunk(int64_t cap);
int tw_count_pairs_sorted(const void* d_x, const int64_t* d_x_off, const void* d_z,
                          const int64_t* d_z_off, int32_t n_shards, int64_t max_nx,
                          int64_t max_nz, int32_t dtype, int32_t pred, void* d_work,
                          uint64_t* d_out, void* stream);
/* ---- Variance components (extension; not in the reference, whose only variances are the
 * closed forms of its Bernoulli model, estimation-experiment/main.py:10-27, :103-104): exact
 * integer moments of the per-point pair counts of every shard, all shards in one launch with any
 * mix of sizes (csrc/moments.hip).  With g_ij = 1{x_i > z_j} (TW_PRED_GT) or 2*1{x_i > z_j} +
 * 1{x_i == z_j} (TW_PRED_HALF), a_i = sum_j g_ij and b_j = sum_i g_ij over shard s,
 *   d_out[4 s + 0 .. 3] = { S = sum a_i, A2 = sum a_i^2, B2 = sum b_j^2, Q = sum g_ij^2 }
 * as uint64; S is tw_count_pairs' count.  The caller keeps n (u m)^2 and m (u n)^2 below 2^64
 * per shard (u = 1 or 2, the predicate's unit).  Layout and arguments as tw_count_pairs; d_work:
 * device scratch of tw_pair_moments_work_bytes(n_shards, total_nx, total_nz) bytes (total_* =
 * off[n_shards] - off[0]), read by the sorted algorithm only.  Deterministic (integer sums). */
int64_t tw_pair_moments_work_bytes(int32_t n_shards, int64_t total_nx, int64_t total_nz);
int tw_pair_moments(const void* d_x, const int64_t* d_x_off, const void* d_z,
                    const int64_t* d_z_off, int32_t n_shards, int64_t max_nx, int64_t max_nz,
                    int32_t dtype, int32_t pred, void* d_work, uint64_t* d_out, void* stream);
/* The two algorithms of tw_pair_moments, same integers: 1 = all pairs (each lane loops over the
 * other side), 2 = sorted (both sides sorted in chunks, two binary searches per point and
 * chunk), 0 = automatic (the default): sorted when max_nx * max_nz >=
 * TW_MOMENTS_SORTED_MIN_PAIRS.  Process-global A/B hook; results do not depend on it. */
#define TW_MOMENTS_SORTED_MIN_PAIRS (1 << 17)
int tw_pair_moments_set_algo(int32_t algo);

/* One step of est.UnNT's loop with the exact sorted count: the counts of tw_count_pairs_sorted
 * for the current partition — except that d_out must already be zero (accumulated into) — and
 * the NEXT repartition: d_x_next / d_z_next = the scores permuted with key_x / key_z (as
 * tw_permute_pair), d_out_next[0 .. n_next_shards) zeroed.  On the bucket path (every shard's
 * nz <= 16384) the permutation's gathers ride in the count threads of the same launch;
 * otherwise the count, tw_permute_pair and a memset run in turn.  d_x_next == NULL: count only.
 * Replaces the shuffle + UN loop of estimation-experiment/main.py:43-79 like tw_count_pairs_step. */
int tw_count_pairs_sorted_step(const void* d_x, const int64_t* d_x_off, const void* d_z,
                               const int64_t* d_z_off, int32_t n_shards, int64_t max_nx,
                               int64_t max_nz, int32_t dtype, int32_t pred, void* d_work,
                               uint64_t* d_out, int64_t n_x, void* d_x_next, uint64_t key_x,
                               int64_t n_z, void* d_z_next, uint64_t key_z,
                               uint64_t* d_out_next, int32_t n_next_shards, void* stream);
/* T steps of est.UnNT's loop (estimation-experiment/main.py:76-79) with the exact sorted count
 * in ONE call: step t repartitions both samples with keys_x[t] / keys_z[t] (host arrays; step 0
 * starts from d_x / d_z in position order) and counts every shard into d_out[t * n_shards ..]
 * (zeroed by the call); the last partition is written to d_x_out / d_z_out (distinct from the
 * inputs).  Between steps the partition lives in d_work as records {value, position} grouped by
 * destination shard, so a repartition is a streaming pass (csrc/records.h) instead of one random
 * gather per score.  The layout must be prop-SWOR's: d_x_off[s] = min(s * kx, n_x),
 * d_z_off[s] = min(s * kz, n_z).  tw_count_pairs_sorted_steps_work_bytes() returns 0 where the
 * path does not apply (then use tw_count_pairs_sorted_step per step). */
int64_t tw_count_pairs_sorted_steps_work_bytes(int64_t n_x, int64_t n_z, int32_t n_shards,
                                               int64_t max_nz, int32_t dtype, int32_t pred);
int tw_count_pairs_sorted_steps(const void* d_x, const void* d_z, int64_t n_x, int64_t n_z,
                                const int64_t* d_x_off, const int64_t* d_z_off, int32_t n_shards,
                                int64_t kx, int64_t kz, int64_t max_nx, int64_t max_nz,
                                int32_t dtype, int32_t pred, const uint64_t* keys_x,
                                const uint64_t* keys_z, int32_t T, void* d_work,
                                int64_t work_bytes, uint64_t* d_out, void* d_x_out,
                                void* d_z_out, void* stream);
/* Shards with nz <= 16384 (default 1): the count comes from value buckets of z in LDS (an
 * LDS histogram, prefix and scatter, then one bucket scanned per x) instead of sorted chunks +
 * binary searches; the same integers.  1 = equal-depth buckets (the value-range histogram's
 * CDF refines the map), 2 = value-range buckets only, 0 = always sort + search (A/B, tests). */
int tw_count_sorted_set_bucket(int32_t by_bucket);

/* ---- Row A3/A4/A5/A8: incomplete count on given index pairs (replay mode) -------------
 * Replaces cs.UB_indices / UB_pairs / UB (compute_stats.py:22-42): pair p of shard s
 * compares x[d_ix[p]] with z[d_iz[p]] for p in [d_pair_off[s], d_pair_off[s+1]); indices are
 * absolute positions in d_x / d_z (int64, as NumPy randint returns them). */
int tw_count_pairs_idx(const void* d_x, const void* d_z, const int64_t* d_ix,
                       const int64_t* d_iz, const int64_t* d_pair_off, int32_t n_shards,
                       int64_t max_pairs, int32_t dtype, int32_t pred, uint64_t* d_out,
                       void* stream);
/* The same counts as tw_count_pairs_idx with the compares on the 16-bit rank codes of
 * tw_count_pairs_rng_ws held in LDS (shard s spans d_x_off[s]..d_x_off[s+1] and
 * d_z_off[s]..d_z_off[s+1]; an index outside its shard's span compares the scores), so the
 * kernel streams only the indices.  d_work holds tw_count_pairs_rng_work_bytes(n_shards,
 * max_nx, max_nz, dtype, pred) bytes; when that is 0 (shards of >= 65536 values, int64 SUBGT) or
 * d_work == NULL this call runs tw_count_pairs_idx. */
/* Tuning hook of tw_count_pairs_idx_ws: blocks of 1024 threads per shard (0 = the plan's). */
int tw_count_idx_set_parts(int32_t parts);
/* Tuning hook of the int32-index ranked count (16-B aligned index streams): 0 = two 16-B loads of
 * each index stream per thread and batch, pipelined: the next batch is issued before the
 * previous one is compared (default), 1 = the same as nontemporal loads, 2/3 = four loads in one
 * buffer, not pipelined (plain / nontemporal), 4/5 = four loads, pipelined (plain /
 * nontemporal).  Process-global; results do not depend on it. */
int tw_count_idx_set_variant(int32_t v);
int tw_count_pairs_idx_ws(const void* d_x, const int64_t* d_x_off, const void* d_z,
                          const int64_t* d_z_off, int32_t n_shards, int64_t max_nx,
                          int64_t max_nz, const int64_t* d_ix, const int64_t* d_iz,
                          const int64_t* d_pair_off, int64_t max_pairs, int32_t dtype,
                          int32_t pred, void* d_work, int64_t work_bytes, uint64_t* d_out,
                          void* stream);
/* int32-index variants — the 8 B/pair replay contract of SURVEY.md §8(d): the same counts as
 * tw_count_pairs_idx / tw_count_pairs_idx_ws with d_ix / d_iz int32 (absolute positions below
 * 2^31).  They replace the same reference lines (compute_stats.py:22-42); the Python layer
 * narrows NumPy's int64 randint output after its bound check (UB_indices' indexing,
 * compute_stats.py:26-30) whenever both samples have fewer than 2^31 elements. */
int tw_count_pairs_idx32(const void* d_x, const void* d_z, const int32_t* d_ix,
                         const int32_t* d_iz, const int64_t* d_pair_off, int32_t n_shards,
                         int64_t max_pairs, int32_t dtype, int32_t pred, uint64_t* d_out,
                         void* stream);
int tw_count_pairs_idx32_ws(const void* d_x, const int64_t* d_x_off, const void* d_z,
                            const int64_t* d_z_off, int32_t n_shards, int64_t max_nx,
                            int64_t max_nz, const int32_t* d_ix, const int32_t* d_iz,
                            const int64_t* d_pair_off, int64_t max_pairs, int32_t dtype,
                            int32_t pred, void* d_work, int64_t work_bytes, uint64_t* d_out,
                            void* stream);

/* ---- Row A5/A8, device-RNG mode: B pairs per shard drawn on the device ----------------
 * Philox4x32-10(key = seed, counter = (q lo, q hi, shard_base + s, 0)) gives the 4 words
 * (w0, w1, w2, w3) of pairs 2q (i from w0, j from w1) and 2q+1 (w2, w3) of local shard s; a word
 * w maps to [0, n) by Lemire's multiply-shift (w * n) >> 32 with rejection of (w * n) mod 2^32
 * < 2^32 mod n, a rejected word being replaced by the same word of counter word 3 = 1, 2, ...
 * (exactly uniform; with-replacement sampling like UB's randint, compute_stats.py:40-41).
 * Shards of >= 2^32 values: pair p uses counter (p lo, p hi, shard_base + s, 0) and maps
 * (w1:w0), (w3:w2) by 64-bit multiply-high.
 * shard_base = the global index of local shard 0, so draws do not depend on how shards are
 * spread over ranks.  Not bit-comparable with NumPy's stream; statistically equivalent
 * (tests/test_statistics.py). */
int tw_count_pairs_rng(const void* d_x, const int64_t* d_x_off, const void* d_z,
                       const int64_t* d_z_off, int32_t n_shards, int64_t B, uint64_t seed,
                       uint64_t shard_base, int32_t dtype, int32_t pred, uint64_t* d_out,
                       void* stream);

/* The same draws and counts as tw_count_pairs_rng, with the compares on 16-bit rank codes held
 * in LDS (sorted z per shard; c_i = #{z < x_i}, c'_i = #{z <= x_i}, p_j = #{z < z_j}; x > z iff
 * c_i > p_j, x >= z iff c'_i > p_j) instead of random 8-B gathers of the scores.  Applies when
 * every shard has nx, nz < 65536, the codes fit in LDS and pred is GT or HALF: then
 * tw_count_pairs_rng_work_bytes() > 0 and d_work must hold that many bytes; otherwise (or with
 * d_work == NULL) this call runs tw_count_pairs_rng. */
int64_t tw_count_pairs_rng_work_bytes(int32_t n_shards, int64_t max_nx, int64_t max_nz,
                                      int32_t dtype, int32_t pred);
/* Rank codes of tw_count_pairs_rng_ws / tw_count_pairs_idx(32)_ws: 1 (default) = equal-depth
 * value buckets in LDS when every shard has nz <= 16384, 2 = value-range buckets only, 0 =
 * always sort + binary search (A/B and tests; same codes). */
int tw_count_rng_set_codes(int32_t by_bucket);
/* Default mode 3 of tw_count_rng_set_codes (csrc/imagecount.hip): instead of rank codes, each
 * block stages the float32 images of its shard's scores in LDS (round to nearest: monotone) and
 * decides x > z on them, gathering the scores only for pairs whose images are equal (ties, -0/+0,
 * values within a float ulp): the same counts, no codes kernel, no workspace.  Applies when a
 * shard pair's images fit in LDS (4 * (nx + nz) bytes <= 159 KiB) and pred is GT or HALF (or
 * SUBGT on doubles); otherwise the codes path runs (and past it the plain kernel).  Tuning hook:
 * blocks per shard (0 = plan) and 16-B index vectors per stream and batch (1, 2, 4; + 8 =
 * nontemporal index loads; default 9). */
int tw_count_img_set_plan(int32_t parts, int32_t u);
/* Tuning hook: Philox blocks each thread of the device-RNG image kernel draws per iteration
 * (1, 2 — the default — or 4; independent chains for the scheduler).  No effect on results. */
int tw_count_rng_img_set_unroll(int32_t qu);
int tw_count_pairs_rng_ws(const void* d_x, const int64_t* d_x_off, const void* d_z,
                          const int64_t* d_z_off, int32_t n_shards, int64_t max_nx,
                          int64_t max_nz, int64_t B, uint64_t seed, uint64_t shard_base,
                          int32_t dtype, int32_t pred, void* d_work, int64_t work_bytes,
                          uint64_t* d_out, void* stream);
/* One step of cs.UnNBT's loop (compute_stats.py:119-123) in device-RNG mode: the counts of
 * tw_count_pairs_rng_ws for the current partition — except that d_out must already be zero
 * (accumulated into) — and the NEXT repartition: d_x_next = the n_x scores of d_x permuted
 * with key_x, d_z_next likewise (as tw_permute_pair), d_out_next[0 .. n_next_shards) zeroed.
 * On the float32-image path (above) the next repartition's gathers ride in the count threads
 * of the same launch; otherwise the count, tw_permute_pair and a memset run in turn.
 * d_x_next == NULL: count only.  Replaces the repartition + UB loop of compute_stats.py:104-110
 * as tw_count_pairs_step does for est.UnNT. */
int tw_count_pairs_rng_step(const void* d_x, const int64_t* d_x_off, const void* d_z,
                            const int64_t* d_z_off, int32_t n_shards, int64_t max_nx,
                            int64_t max_nz, int64_t B, uint64_t seed, uint64_t shard_base,
                            int32_t dtype, int32_t pred, void* d_work, int64_t work_bytes,
                            uint64_t* d_out, int64_t n_x, void* d_x_next, uint64_t key_x,
                            int64_t n_z, void* d_z_next, uint64_t key_z, uint64_t* d_out_next,
                            int32_t n_next_shards, void* stream);

/* ---- Row A2 (prod/gini) and f1 (conv_AUC): float pair sums, complete -------------------
 * d_out[s] (double) = sum over all pairs of shard s of kern(x_i, z_j).  Deterministic: fixed
 * per-block partial order, then an ordered per-shard reduction.  d_work: n_shards *
 * tw_pair_sum_work_per_shard(max_nx, max_nz) doubles. */
int64_t tw_pair_sum_work_per_shard(int64_t max_nx, int64_t max_nz);
int tw_pair_sum_f64(const double* d_x, const int64_t* d_x_off, const double* d_z,
                    const int64_t* d_z_off, int32_t n_shards, int64_t max_nx, int64_t max_nz,
                    int32_t kern, double margin, double* d_work, double* d_out, void* stream);

/* ---- f1: float pair sums on given index pairs (conv_AUC_deter_pairs, UB_indices prod/gini)
 * d_out[s] = sum_p kern(x[ix_p], z[iz_p]); d_work: n_shards * tw_pair_sum_idx_work_per_shard(max_pairs). */
int64_t tw_pair_sum_idx_work_per_shard(int64_t max_pairs);
int tw_pair_sum_idx_f64(const double* d_x, const double* d_z, const int64_t* d_ix,
                        const int64_t* d_iz, const int64_t* d_pair_off, int32_t n_shards,
                        int64_t max_pairs, int32_t kern, double margin, double* d_work,
                        double* d_out, void* stream);
/* int32 indices; d_count (nullable, uint64 per shard): the same pass also counts x > z — the
 * fixed-pair br_AUC of evaluation_step (UB_pairs(kernel="AUC"), make_exps.py:162-168) beside
 * its hinge mean bc_AUC (conv_AUC_deter_pairs, compute_stats.py:137-144), one read of the
 * monitor pairs for both. */
int tw_pair_sum_idx32_f64(const double* d_x, const double* d_z, const int32_t* d_ix,
                          const int32_t* d_iz, const int64_t* d_pair_off, int32_t n_shards,
                          int64_t max_pairs, int32_t kern, double margin, double* d_work,
                          double* d_out, uint64_t* d_count, void* stream);

/* ---- Row L1: pairwise hinge gradient, all shards in one launch ------------------------
 * Replaces grad_inc_block(w, B, margin)(X_s, Z_s) (compute_stats.py:146-162) for every shard
 * of UN_split (compute_stats.py:44-46).  X: (n_X, d) row-major doubles, Z: (n_Z, d).
 * Shard s, pair b: rx = d_rows_x[s*kx + d_ix[s*B+b]], rz = d_rows_z[s*kz + d_iz[s*B+b]]
 * (SWR_divide row draws composed with the per-block randint draws, compute_stats.py:48-54,
 * :155-156); d_rows_x / d_rows_z may be NULL meaning identity (shard = whole array).
 * diff = Z[rz] - X[rx]; S = diff . w + margin; d_out[s*d + j] = (sum_{b: S_b > 0} diff_bj) / B,
 * summed over b in order (as NumPy's axis-0 reduce does). */
int tw_hinge_grad(const double* d_X, const double* d_Z, int64_t d, const int64_t* d_rows_x,
                  int64_t kx, const int64_t* d_rows_z, int64_t kz, const int64_t* d_ix,
                  const int64_t* d_iz, int32_t n_shards, int64_t B, const double* d_w,
                  double margin, double* d_out, void* stream);

/* Same for either loss: d_out[s*d + j] = (sum_b weight_b * diff_bj) / B in row order, with
 * weight 1{S_b > 0} (hinge: filtered rows only, exactly as above) or sigma(S_b) (logistic). */
int tw_pair_grad(const double* d_X, const double* d_Z, int64_t d, const int64_t* d_rows_x,
                 int64_t kx, const int64_t* d_rows_z, int64_t kz, const int64_t* d_ix,
                 const int64_t* d_iz, int32_t n_shards, int64_t B, const double* d_w,
                 double margin, int32_t loss, double* d_out, void* stream);

/* Sign audit (SURVEY.md §7 "count and report" the hinge-filter flips): tw_pair_grad plus
 * d_scores[s*B + b] = S_b = diff_b . w + margin exactly as the kernel computed it (the generic
 * kernel; its narrow and wide paths sum the dot product in the orders of the streaming and fused
 * kernels).  The reference decides the filter on BLAS's S (compute_stats.py:158-159); the
 * caller compares the signs (tuplewise.learning.learning_process(..., sign_audit=[])). */
int tw_pair_grad_audit(const double* d_X, const double* d_Z, int64_t d, const int64_t* d_rows_x,
                       int64_t kx, const int64_t* d_rows_z, int64_t kz, const int64_t* d_ix,
                       const int64_t* d_iz, int32_t n_shards, int64_t B, const double* d_w,
                       double margin, int32_t loss, double* d_out, double* d_scores,
                       void* stream);

/* ---- Complete-block gradient (extension; BASELINE.json north_star item (2)) -------------
 * The same surrogate's gradient over ALL kx*kz pairs of each shard, computed as per-point
 * pair-coefficient reductions followed by X^T c (csrc/complete_grad.hip):
 *   sx_i = X[rx_i].w, sz_j = Z[rz_j].w, S_ij = sz_j - sx_i + margin,
 *   a_j = sum_i phi'(S_ij), b_i = sum_j phi'(S_ij)  (phi' = 1{S>0} hinge, sigma(S) logistic),
 *   d_out[s*d + c] = (sum_j a_j Z[rz_j][c] - sum_i b_i X[rx_i][c]) / (kx*kz).
 * Rows as tw_hinge_grad (d_rows_* NULL = shard s owns rows [s*k, (s+1)*k)).  d_work: device
 * scratch of tw_pair_grad_complete_work_bytes(n_shards, kx, kz, d) bytes.  Deterministic
 * (fixed summation orders); not in the reference (its learner samples B pairs). */
int64_t tw_pair_grad_complete_work_bytes(int32_t n_shards, int64_t kx, int64_t kz, int64_t d);
int tw_pair_grad_complete(const double* d_X, const double* d_Z, int64_t d,
                          const int64_t* d_rows_x, int64_t kx, const int64_t* d_rows_z,
                          int64_t kz, int32_t n_shards, const double* d_w, double margin,
                          int32_t loss, void* d_work, double* d_out, void* stream);
/* Hinge coefficients are counts; by default they come from binary searches with the exact
 * floating-point predicate over each shard's sorted scores (S is monotone in each score), the
 * same integers as the pair-by-pair sums in O(k log k); logistic coefficients come from one
 * pass over the pairs (each sigma(S_ij) feeds a_j and b_i).  on = 0 selects the two-pass
 * pair-by-pair kernels (kept for A/B checks). */
int tw_pair_grad_complete_set_search(int32_t on);

/* ---- Row L1/A9, device-RNG mode (no host RNG in the loop; graph-capturable) -----------
 * Draws are Philox4x32-10(key = seed, counter = (index, shard, step lo, tag | step hi)) with
 * step = *d_step (device memory, advanced by tw_sgd_update), mapped by 64-bit multiply-high;
 * the shard word is shard_base + local shard, so draws follow GLOBAL shard indices and a
 * run spread over ranks draws exactly what a single GPU draws:
 * tw_hinge_grad_rng: pair b of shard s -> (ix, iz) in [0,kx) x [0,kz) (tag 0x80000000);
 * tw_swr_rows_rng:   d_rows[s*k + t] in [0, n), side 0 = X rows (tag 0x40000000), 1 = Z rows
 *                    (tag 0x20000000) — SWR_divide (compute_stats.py:48-54) on the device.
 * Statistically equivalent to the reference's NumPy draws, not bit-comparable; exactly
 * reproducible from (seed, step) and checked against oracle/oracle.py's restatement. */
int tw_hinge_grad_rng(const double* d_X, const double* d_Z, int64_t d, const int64_t* d_rows_x,
                      int64_t kx, const int64_t* d_rows_z, int64_t kz, int32_t n_shards,
                      int64_t B, const double* d_w, double margin, uint64_t seed,
                      const uint64_t* d_step, int32_t shard_base, double* d_out, void* stream);
/* Tuning hook for 32 < d <= 512 rows: 0 = the streaming kernel (default: two register stages,
 * 16-pair chunks), 1 = the unpipelined kernel, 2 = the burst-pipelined kernel (32-pair chunks).
 * Process-global; all give identical bits. */
int tw_hinge_set_variant(int32_t legacy_wide);
int tw_pair_grad_rng(const double* d_X, const double* d_Z, int64_t d, const int64_t* d_rows_x,
                     int64_t kx, const int64_t* d_rows_z, int64_t kz, int32_t n_shards, int64_t B,
                     const double* d_w, double margin, int32_t loss, uint64_t seed,
                     const uint64_t* d_step, int32_t shard_base, double* d_out, void* stream);
int tw_swr_rows_rng(int64_t* d_rows, int32_t n_shards, int64_t k, int64_t n, uint64_t seed,
                    const uint64_t* d_step, int32_t side, int32_t shard_base, void* stream);

/* ---- Row L2: update of learning_process (make_exps.py:130-141) ------------------------
 * g = mean_s(d_grads[s]) + reg * w  (shards summed in order, then / n_shards — np.mean axis 0)
 * momentum: dw = momentum * dw + lr * g;  SGD (momentum < 0): dw = lr * g;   w = w - dw.
 * d_step (nullable): device-RNG step counter, incremented once. */
int tw_sgd_update(double* d_w, double* d_dw, const double* d_grads, int32_t n_shards, int64_t d,
                  double reg, double lr, double momentum, uint64_t* d_step, void* stream);
/* Same update from (d_w_in, d_dw_in) into (d_w, d_dw) (may be the same buffers); the step
 * counter (nullable) advances by step_inc.  Ends a segment of tw_sgd_step launches. */
int tw_sgd_update_to(const double* d_w_in, const double* d_dw_in, double* d_w, double* d_dw,
                     const double* d_grads, int32_t n_shards, int64_t d, double reg, double lr,
                     double momentum, uint64_t* d_step, int32_t step_inc, void* stream);

/* ---- Rows L1 + L2 fused: one launch per SGD step (narrow rows, d <= 32, n_shards*d <= 4096;
 * tw_sgd_step_fusable says whether a shape qualifies).  The launch first applies the update of
 * the PREVIOUS step (d_grads_in, d_w_in, d_dw_in -> w, written by block 0 to d_w_out/d_dw_out;
 * every block computes it, so no grid synchronisation), then computes this step's per-shard
 * gradients with it into d_grads_out.  d_grads_in == NULL: no pending update (w = d_w_in).
 * Draws: replay (d_ix, d_iz) or device RNG at step *d_step + step_off (the counter itself is
 * advanced by the tw_sgd_update_to that ends the segment).  A segment of k steps is
 *   step 0: in (w0, -, -) -> grads G0;   step j>0: in (W[j-1&1], DW[j-1&1], G[j-1&1]) ->
 *   out (W[j&1], DW[j&1], G[j&1]);  then tw_sgd_update_to(W[k-1&1], DW[k-1&1] -> w0, dw0,
 *   G[k-1&1], step_inc = k)
 * (ping-pong slots, slot 0 = w0/dw0): the same bits as k tw_pair_grad(_rng) + tw_sgd_update
 * pairs, with k + 1 launches instead of 2k. */
int tw_sgd_step_fusable(int64_t d, int32_t n_shards);
int tw_sgd_step(const double* d_X, const double* d_Z, int64_t d, const int64_t* d_rows_x,
                int64_t kx, const int64_t* d_rows_z, int64_t kz, const int64_t* d_ix,
                const int64_t* d_iz, int32_t n_shards, int64_t B, double margin, int32_t loss,
                uint64_t seed, const uint64_t* d_step, int32_t step_off, int32_t shard_base,
                const double* d_w_in, const double* d_dw_in, const double* d_grads_in, double reg,
                double lr, double momentum, double* d_w_out, double* d_dw_out,
                double* d_grads_out, void* stream);

/* A segment of nsteps narrow-row SGD steps (d <= 32; the steps tw_sgd_step launches one by
 * one) in ONE persistent launch (csrc/sgdseg.hip k_sgd_segment_narrow): one block per shard,
 * all co-resident, one grid barrier per step, the update recomputed in every block from the
 * published shard gradients (slots d_grads0 / d_grads1 by step parity).  On return d_w_out /
 * d_dw_out hold the state after the segment's last update and the last step's gradients are
 * in slot (nsteps-1) & 1: apply them with tw_sgd_update_to(d_w_out, d_dw_out -> w, dw,
 * step_inc = nsteps).  Draws: d_ix/d_iz + step k * draw_stride (replay) or device RNG at
 * *d_step + k.  d_ctl: 2 words, zeroed once by the caller — the arrival counter (the kernel
 * leaves it at zero again) and a sticky abort word (set when a bounded barrier wait expired).
 * The residency check (tw_sgd_segment_narrow_ok) is the caller's, once, outside any stream
 * capture: this entry only checks shapes.  Same bits as tw_sgd_step per step.
 * make_exps.py:122-141 with compute_stats.py:146-162. */
int tw_sgd_segment_narrow_ok(int64_t d, int32_t n_shards, int64_t B);
int tw_sgd_segment_narrow(const double* d_X, const double* d_Z, int64_t d,
                          const int64_t* d_rows_x, int64_t kx, const int64_t* d_rows_z, int64_t kz,
                          const int64_t* d_ix, const int64_t* d_iz, int64_t draw_stride,
                          int32_t n_shards, int64_t B, double margin, int32_t loss, uint64_t seed,
                          const uint64_t* d_step, int32_t shard_base, int32_t nsteps,
                          const double* d_w_in, const double* d_dw_in, double reg, double lr,
                          double momentum, double* d_grads0, double* d_grads1, double* d_w_out,
                          double* d_dw_out, uint32_t* d_ctl, void* stream);
/* tw_sgd_segment_narrow replaying through reshuffles: d_rows_x / d_rows_z are stacks of SWR
 * row tables tab_x / tab_z words apart (>= n_shards * kx / kz), and step k of the segment
 * reads table (tab_phase + k) / tab_mod — the segment starts at step tab_phase of a reshuffle
 * period of tab_mod steps (0 <= tab_phase < tab_mod), table 0 being the tables in force at its
 * start (learning_process's SWR_divide every `mod` steps, make_exps.py:123-125, without
 * ending the segment there). */
int tw_sgd_segment_narrow_tables(
    const double* d_X, const double* d_Z, int64_t d, const int64_t* d_rows_x, int64_t kx,
    const int64_t* d_rows_z, int64_t kz, int64_t tab_x, int64_t tab_z, int64_t tab_phase,
    int64_t tab_mod, const int64_t* d_ix, const int64_t* d_iz, int64_t draw_stride,
    int32_t n_shards, int64_t B, double margin, int32_t loss, uint64_t seed,
    const uint64_t* d_step, int32_t shard_base, int32_t nsteps, const double* d_w_in,
    const double* d_dw_in, double reg, double lr, double momentum, double* d_grads0,
    double* d_grads1, double* d_w_out, double* d_dw_out, uint32_t* d_ctl, void* stream);
/* tw_sgd_segment_narrow in device-RNG mode with the SWR row tables drawn IN the kernel: the
 * row of draw position a of shard s at step counter c is the one tw_swr_rows_rng drew at the
 * last reshuffle, counter rc = c - (c - swr_base) % swr_mod (reshuffles every swr_mod steps
 * from swr_base: make_exps.py:123-125), so one launch runs through any number of reshuffles.
 * Same bits as tw_swr_rows_rng at every reshuffle + tw_sgd_segment_narrow between them. */
int tw_sgd_segment_narrow_swr(const double* d_X, const double* d_Z, int64_t d, int64_t n_X,
                              int64_t n_Z, int64_t kx, int64_t kz, int32_t n_shards, int64_t B,
                              double margin, int32_t loss, uint64_t seed, const uint64_t* d_step,
                              int32_t shard_base, int32_t nsteps, int64_t swr_mod,
                              uint64_t swr_base, const double* d_w_in, const double* d_dw_in,
                              double reg, double lr, double momentum, double* d_grads0,
                              double* d_grads1, double* d_w_out, double* d_dw_out,
                              uint32_t* d_ctl, void* stream);
/* evaluation_step's FIXED_PAIRS statistics (make_exps.py:143-190) for small problems in two
 * launches: the scores A @ w of train X (n_trX x d), train Z, test X, test Z into d_scores
 * (concatenated, k_gemv's arithmetic), then the monitor pairs' surrogate sum and AUC count
 * (d_ix/d_iz: n_pairs int32 row indices; d_offs = {0, n_pairs, 0, n_teX, 0, n_teZ} on the
 * device) and all test pairs' surrogate sum and AUC count, reduced in one launch: d_out =
 * {monitor sum, monitor count (uint64 bits), test sum, test count (uint64 bits)} — the same
 * values as tw_gemv_f64 + tw_pair_sum_idx32_f64 + tw_pair_sum_f64 + tw_count_pairs.  d_work /
 * d_cwork: tw_eval_small_work(...) entries each; d_ticket: one zeroed word (left zero). */
int64_t tw_eval_small_work(int64_t n_pairs, int64_t n_test_x, int64_t n_test_z);
int tw_eval_small(const double* d_trX, int64_t n_trX, const double* d_trZ, int64_t n_trZ,
                  const double* d_teX, int64_t n_teX, const double* d_teZ, int64_t n_teZ,
                  int64_t d, const double* d_w, const int32_t* d_ix, const int32_t* d_iz,
                  int64_t n_pairs, const int64_t* d_offs, int32_t kern, double margin,
                  double* d_scores, double* d_work, uint64_t* d_cwork, uint32_t* d_ticket,
                  double* d_out, void* stream);
/* tw_pair_grad_rng with the SWR rows drawn in the kernel (reshuffles every swr_mod steps from
 * counter swr_base; the rows of tw_swr_rows_rng at the last reshuffle): the per-step gradient
 * of wide rows (C5) needs no row tables and no table-drawing launch per reshuffle. */
int tw_pair_grad_rng_swr(const double* d_X, const double* d_Z, int64_t d, int64_t n_X,
                         int64_t n_Z, int64_t kx, int64_t kz, int32_t n_shards, int64_t B,
                         const double* d_w, double margin, int32_t loss, uint64_t seed,
                         const uint64_t* d_step, int32_t shard_base, int64_t swr_mod,
                         uint64_t swr_base, double* d_out, void* stream);
/* ---- The hinge surrogate over ALL pairs of each shard in O((n + m) log m) (f64 scores):
 * d_out[s] = sum_{i,j} max(fl(fl(z_j - x_i) + margin), 0) — cs.conv_AUC's sum
 * (compute_stats.py:129-135) as evaluation_step's tc_AUC (make_exps.py:167-168) and
 * SAME_AS_BATCH's bc_AUC (:154-157) need it.  For each x the positive terms are the top c of
 * the shard's sorted z (a binary search with the exact predicate), summed from double-double
 * prefix sums: the exact sum of the terms rounded once (vs NumPy's pairwise sum of rounded
 * terms: ~1e-15 relative).  NaN / +-inf follow NumPy's elementwise semantics (NaN or +inf
 * results).  Empty shards give 0.  d_work: tw_pair_hinge_sum_sorted_work_bytes bytes. */
int64_t tw_pair_hinge_sum_sorted_work_bytes(int32_t n_shards, int64_t max_nx, int64_t max_nz);
int tw_pair_hinge_sum_sorted(const double* d_x, const int64_t* d_x_off, const double* d_z,
                             const int64_t* d_z_off, int32_t n_shards, int64_t max_nx,
                             int64_t max_nz, double margin, void* d_work, double* d_out,
                             void* stream);

/* ---- f1: scores = A @ w for a row-major (n, d) matrix (evaluation_step, make_exps.py:163,
 * :170-171).  d <= 32: row dot products in index order; d > 32: see tw_gemv_set_variant. */
int tw_gemv_f64(const double* d_A, int64_t n, int64_t d, const double* d_w, double* d_out,
                void* stream);
/* Tuning hook: 1 (default) computes rows of d > 32 one wave per row (lane-strided partial dots
 * + a fixed butterfly, coalesced 16-B loads; 16-B aligned A and w), 0 = a thread per row in
 * index order.  Scores may differ in the last ulp between the two (BLAS's order differs too). */
int tw_gemv_set_variant(int32_t rows);

/* ---- Row A6/A9/(e): repartition on the device ----------------------------------------
 * Keyed pseudo-random permutation of [0, n): a 6-round Feistel network over the smallest
 * even-bit power-of-two domain >= n, with cycle walking (a bijection on [0, n)).
 * tw_permute_scatter: d_out[perm(i)] = d_in[i] for i in [0, n) (8-byte elements).
 * tw_perm_index: d_perm[i] = perm(i). */
int tw_permute_scatter(const void* d_in, void* d_out, int64_t n, uint64_t key, void* stream);
/* Both samples of one repartition in one launch: X (n elements, key_x) and Z (m, key_z),
 * each exactly as tw_permute_scatter. */
int tw_permute_pair(const void* d_x_in, void* d_x_out, int64_t n, uint64_t key_x,
                    const void* d_z_in, void* d_z_out, int64_t m, uint64_t key_z, void* stream);
int tw_perm_index(int64_t* d_perm, int64_t n, int64_t base, int64_t n_total, uint64_t key,
                  void* stream);

/* ---- (e) multi-rank repartition: counting sort of this rank's elements by destination rank
 * (dest = perm / n_loc, G <= 64 ranks), packed as 16-byte records {value bits, dest-local
 * position + pos_base} for an all-to-all(v); the receiver scatters the records into its local
 * array.  tw_rank_histogram: d_counts[g] = #elements bound for rank g.  tw_source_histogram:
 * d_counts[q] = #positions in [base, base+n) whose source perm^-1(p) (the permutation of
 * [0, n_total) keyed by `key`, as tw_perm_index) lies on rank q = source / n_loc — what this
 * rank receives from q, known without a message.  tw_bucket_scatter: record of element i goes
 * to d_send[2*(d_start[dst] + k)], k a per-destination slot reserved per block (d_cursor: G
 * uint64 of scratch); pos_base lets two arrays share one record buffer (e.g. Z positions
 * offset by n_loc of X).  tw_scatter_records: d_out[rec.pos] = rec.value for m records. */
int tw_rank_histogram(const int64_t* d_perm, int64_t n, int64_t n_loc, int32_t G,
                      uint64_t* d_counts, void* stream);
int tw_source_histogram(int64_t n, int64_t base, int64_t n_total, uint64_t key, int64_t n_loc,
                        int32_t G, uint64_t* d_counts, void* stream);
int tw_bucket_scatter(const int64_t* d_perm, const void* d_vals, int64_t n, int64_t n_loc,
                      int32_t G, const int64_t* d_start, uint64_t* d_cursor, int64_t pos_base,
                      void* d_send, void* stream);
int tw_scatter_records(const void* d_rec, int64_t m, void* d_out, void* stream);
/* The same exchange for BOTH samples of one repartition in two launches and without a
 * permutation array (what ShardedSample runs).  Rank `rank` owns global X positions
 * [rank*n_loc, (rank+1)*n_loc) of G*n_loc (key_x) and Z positions likewise (m_loc, key_z).
 * tw_exchange_counts: d_counts (4G uint64) = [send X | receive X | send Z | receive Z] per
 *   rank; zeroes d_cursor (2G uint64 of scratch).
 * tw_exchange_pack: d_send ((n_loc+m_loc) records of 16 bytes) grouped by destination rank g,
 *   each group [X records | Z records] in the order of the send counts; a record is {value
 *   bits, destination-local position}, Z positions offset by n_loc, so the receiver scatters
 *   everything into one [X | Z] array with tw_scatter_records. */
/* Tuning hook: grid cap (blocks) of tw_exchange_counts / tw_exchange_pack /
 * tw_scatter_records, which run beside a count kernel (0 = default).  Results do not
 * depend on it. */
int tw_exchange_set_grid(int32_t blocks);
int tw_exchange_counts(int64_t n_loc, int64_t m_loc, int32_t rank, int32_t G, uint64_t key_x,
                       uint64_t key_z, uint64_t* d_counts, uint64_t* d_cursor, void* stream);
int tw_exchange_pack(const void* d_x, int64_t n_loc, const void* d_z, int64_t m_loc, int32_t rank,
                     int32_t G, uint64_t key_x, uint64_t key_z, const uint64_t* d_counts,
                     uint64_t* d_cursor, void* d_send, void* stream);
/* Fixed-capacity variant (the default exchange of ShardedSample): ONE forward-permutation pass,
 * no count pass and no host round trip.  d_send holds G buckets of (1 + cap) records: bucket g =
 * [header {count, 0} | records {value bits, position at rank g (Z offset by n_loc)}], so the
 * all-to-all is an equal-split one (G*(1+cap) records each way).  d_cursor (G uint64) must be
 * zero on the first call; it is left zero for the next.  A bucket over cap sets *d_flag (the
 * records past cap are dropped): the caller must check the flag before using the result.
 * tw_scatter_buckets: for every received bucket, d_out[pos] = value for its first
 * min(header, cap) records; a header over cap or a position outside [0, n_out) sets *d_flag.
 * Replaces the same reference loop as tw_exchange_pack (compute_stats.py:64-67 per rank). */
int tw_exchange_pack_fixed(const void* d_x, int64_t n_loc, const void* d_z, int64_t m_loc,
                           int32_t rank, int32_t G, uint64_t key_x, uint64_t key_z, int64_t cap,
                           uint64_t* d_cursor, void* d_send, int32_t* d_flag, void* stream);
int tw_scatter_buckets(const void* d_recv, int32_t G, int64_t cap, void* d_out, int64_t n_out,
                       int32_t* d_flag, void* stream);

/* ---- (e): row exchange for the row-partitioned learning layout ------------------------
 * Replaces the row copies of SWR_divide (compute_stats.py:48-54) when X is split by rows over
 * G ranks.  d_rows: the M = N*k global row indices of all N shards (shard-major; identical on
 * every rank).  Requester q owns positions [q*M_q, (q+1)*M_q).  This rank owns matrix rows
 * [lo, hi), stored row-major as d_part ((hi-lo) x d).
 * tw_row_route_counts: d_counts[q] = #positions of q whose row lies in [lo, hi).
 * tw_row_pack: one record of d+1 doubles per such position into d_send — the row, then the
 *   requester-local position bit-cast to a double — requester q's records occupying
 *   [d_start[q], d_start[q] + d_counts[q]) (order inside a bucket unspecified); d_cursor: G
 *   int64 of scratch.  G <= 1024.
 * tw_row_unpack: d_out[pos*d + c] = record[c] for m received records. */
int tw_row_route_counts(const int64_t* d_rows, int64_t M, int64_t M_q, int64_t lo, int64_t hi,
                        int32_t G, int64_t* d_counts, void* stream);
int tw_row_pack(const int64_t* d_rows, int64_t M, int64_t M_q, int64_t lo, int64_t hi, int32_t G,
                const double* d_part, int64_t d, const int64_t* d_start, int64_t* d_cursor,
                double* d_send, void* stream);
int tw_row_unpack(const double* d_rec, int64_t m, int64_t d, double* d_out, void* stream);
/* Remote rows only (the learning layout's default): this rank's matrix is [partition |
 * receive area], and its row tables point into it — owned draws at their partition row, the
 * others where the exchange lands them.  Nothing owned is copied; at G = 1 nothing moves.
 * tw_row_route_remote_counts: tw_row_route_counts with d_counts[me] = 0 (me: this rank).
 * tw_row_pack_remote: requester q's bucket starts at word d_start[q] of d_send and holds
 *   d_count[q] rows (d doubles each; order unspecified) followed by their requester-local
 *   positions (bit-cast int64), padded by the caller to whole rows: ceil(d_count[q] / d) * d
 *   words.  d_cursor: G int64 of scratch.
 * tw_row_table_local: d_table[i] = d_rows[i] - lo for this rank's M_q positions whose row it
 *   owns (d_rows: its own slice of the draws), -1 for the others.
 * tw_row_table_remote: for the `total` records received (source g's bucket at word
 *   d_rstart[g] of d_recv, d_rcount[g] records, d_rprefix[g] = sum of the counts before g):
 *   d_table[position] = base + d_rstart[g] / d + j for record j — d_recv being the receive
 *   area of the matrix at row `base` (the partition's row count); a position outside
 *   [0, table_len), or a record past recv_len words, is not used and raises *d_bad (position
 *   + 1, or 2^62: a protocol error the caller reports; d_bad may be NULL). */
int tw_row_route_remote_counts(const int64_t* d_rows, int64_t M, int64_t M_q, int64_t lo,
                               int64_t hi, int32_t G, int32_t me, int64_t* d_counts,
                               void* stream);
int tw_row_pack_remote(const int64_t* d_rows, int64_t M, int64_t M_q, int64_t lo, int64_t hi,
                       int32_t G, int32_t me, const double* d_part, int64_t d,
                       const int64_t* d_start, const int64_t* d_count, int64_t* d_cursor,
                       double* d_send, void* stream);
int tw_row_table_local(const int64_t* d_rows, int64_t M_q, int64_t lo, int64_t hi,
                       int64_t* d_table, void* stream);
int tw_row_table_remote(const double* d_recv, int32_t G, const int64_t* d_rstart,
                        const int64_t* d_rcount, const int64_t* d_rprefix, int64_t total,
                        int64_t d, int64_t base, int64_t* d_table, int64_t table_len,
                        int64_t recv_len, int64_t* d_bad, void* stream);

/* ---- (e) single-process multi-device communicator (RCCL over xGMI) --------------------
 * The reference's workers are one serial in-process loop (compute_stats.py:71-91,
 * estimation-experiment/main.py:48-68), so the drop-in API drives all of the node's GPUs
 * from ONE process: a call's blocks are spread over the devices and their
 * per-block integers combined by an all-gather.  RCCL is bound at run time (the copy already
 * in the process, else the system librccl.so.1); without it tw_comm_init returns TW_ERR_HIP
 * and the caller gathers on the host (same integers).
 * tw_comm_init: one communicator over ndev distinct devices (ncclCommInitAll) -> *out_comm.
 * tw_allgather_u64 / _f64: for every k, device devs[k] sends count words from d_send[k] and
 *   receives ndev*count words (rank order) into d_recv[k], on streams[k] (hipStream_t of
 *   device k); pointer arrays are host arrays of ndev device pointers. */
int tw_comm_init(int32_t ndev, const int32_t* devs, int32_t* out_comm);
int tw_comm_destroy(int32_t comm);
int tw_allgather_u64(int32_t comm, const uint64_t* const* d_send, uint64_t* const* d_recv,
                     int64_t count, void* const* streams);
int tw_allgather_f64(int32_t comm, const double* const* d_send, double* const* d_recv,
                     int64_t count, void* const* streams);
/* Failure detection (the one entry point here that waits): block until the
 * collectives enqueued on streams[k] (one per device of the communicator) complete, polling
 * ncclCommGetAsyncError on every device's communicator; an RCCL error, a failed stream or
 * timeout_ms (<= 0: the tw_comm_set_timeout default, 60 s) aborts the communicator
 * (ncclCommAbort) and returns TW_ERR_HIP — later calls on the handle fail at once, and the
 * caller gathers on the host instead.  Replaces the wait the reference never needed: its
 * workers are a serial loop (compute_stats.py:71-92). */
int tw_comm_wait(int32_t comm, void* const* streams, int64_t timeout_ms);
int tw_comm_set_timeout(int64_t ms);
/* The deadline of the work queued on the streams BEFORE the last collective (default 600 s):
 * tw_comm_wait waits for it first, outside the collective's own deadline, and aborts the
 * communicator if it has not drained by then (a wedged stream ends in an error, not a hang). */
int tw_comm_set_prior_timeout(int64_t ms);

/* ---- (e) learning over ranks: device-resident gradient exchange (round 5, csrc/peer.hip,
 * csrc/peer.h).  Replaces the per-step all-gather of the shard partials between the gradient
 * and the update launches (the shard mean of make_exps.py:126-141 / compute_stats.py:44-46,
 * split over ranks) by GPU-to-GPU stores into one peer buffer per rank, IPC-mapped into the
 * others.  tw_peer_buffer_bytes: the buffer size for n_total shards of d columns (-1: bad
 * sizes).  tw_peer_alloc: a zeroed UNCACHED device buffer (*out_uncached = 1); fails with
 * TW_ERR_HIP when the driver cannot give uncached memory (no cached fallback: stale lines).  tw_peer_handle / tw_peer_open / tw_peer_close: the 64-byte
 * IPC handle of a buffer, mapped into another process (hipIpcMemLazyEnablePeerAccess).
 * d_peer_bases below: G device addresses in rank order (this rank's own buffer at `rank`). */
int64_t tw_peer_buffer_bytes(int32_t n_total, int64_t d);
int tw_peer_alloc(int64_t bytes, void** d_out, int32_t* out_uncached);
int tw_peer_free(void* d_ptr);
int tw_peer_handle(void* d_ptr, uint8_t* out_handle);
int tw_peer_open(const uint8_t* handle, void** d_out);
int tw_peer_close(void* d_ptr);
/* Setup handshake: tw_peer_hello stores `token` into this rank's hello word of every rank's
 * buffer (and waits for it); after a host barrier over the ranks, tw_peer_check sets *out_ok
 * = 1 when its own buffer's G hello words all hold `token`. */
int tw_peer_hello(void* const* d_peer_bases, int32_t G, int32_t rank, uint64_t token,
                  void* stream);
int tw_peer_check(void* d_my_base, int32_t G, uint64_t token, int32_t* out_ok);
/* Per-step form, ONE launch after the gradient launch, parity par = step & 1: this rank's
 * `words` partial words (its shards' rows, global offset offset_words = shard_base * d) stored
 * into every rank's slot and the launch's arrivals added to every rank's counter; then the
 * launch waits (bounded: 20 s, *d_abort raised on timeout) until all G ranks' arrivals are in
 * and applies tw_sgd_update's arithmetic to the n_total x d slot (same bits), d_step advanced
 * by one when given.  Uneven shard splits need nothing more: the arrivals per rank depend on
 * d only. */
int tw_peer_step(const double* d_grads_loc, int64_t words, int64_t offset_words,
                 void* const* d_peer_bases, int32_t G, int32_t rank, int32_t n_total, int64_t d,
                 int32_t par, double* d_w, double* d_dw, double reg, double lr, double momentum,
                 uint64_t* d_step, uint32_t* d_abort, void* stream);
/* Column-owned per-step form (round 6): tw_peer_step's arguments and the same w / dw bits on
 * every rank; rank p sums and updates only columns [p d / G, (p+1) d / G) (each rank pushes
 * each partial column to its owner only, owners publish their updated columns to every rank).
 * words and offset_words are whole rows (multiples of d). */
int tw_peer_step_cols(const double* d_grads_loc, int64_t words, int64_t offset_words,
                      void* const* d_peer_bases, int32_t G, int32_t rank, int32_t n_total,
                      int64_t d, int32_t par, double* d_w, double* d_dw, double reg, double lr,
                      double momentum, uint64_t* d_step, uint32_t* d_abort, void* stream);
/* The narrow persistent segment (tw_sgd_segment_narrow) over ranks: this rank's n_shards
 * blocks (global shards shard_base..) push every step's gradients into every rank's peer
 * buffer and wait for all n_total shards on their own; the last update is applied in the
 * launch (d_w / d_dw in place; d_step += nsteps when given).  Replay draws d_ix / d_iz: this
 * rank's first shard's rows (draw_stride per step); device RNG: d_ix = d_iz = NULL, and
 * swr_mod > 0 draws the SWR rows in the kernel (else the row tables d_rows_x / d_rows_z).
 * d_ctl[1]: the abort word. */
int tw_sgd_segment_narrow_peer(const double* d_X, const double* d_Z, int64_t d,
                               const int64_t* d_rows_x, int64_t kx, const int64_t* d_rows_z,
                               int64_t kz, const int64_t* d_ix, const int64_t* d_iz,
                               int64_t draw_stride, int32_t n_shards, int64_t B, double margin,
                               int32_t loss, uint64_t seed, uint64_t* d_step,
                               int32_t shard_base, int32_t nsteps, int64_t n_X, int64_t n_Z,
                               int64_t swr_mod, double* d_w, double* d_dw, double reg,
                               double lr, double momentum, uint32_t* d_ctl,
                               void* const* d_peer_bases, int32_t G, int32_t rank,
                               int32_t n_total, void* stream);

/* ---- f2: bulk draws of NumPy's legacy global RNG (host code, no GPU) ------------------
 * key (624 words) / pos: the MT19937 state of np.random.get_state(), advanced in place.
 * tw_np_randint_batch: n_calls consecutive RandomState.randint(low[c], high[c], cnt[c]) calls
 * (int64 output, NumPy's masked-rejection algorithm), values concatenated into out; returns
 * 0, or 1 when a range is empty (high <= low).  Replaces the per-shard randint calls of
 * grad_inc_block (compute_stats.py:155-156) and SWR_divide (:52-53) in replay mode.
 * tw_np_mt_next32: the raw genrand_int32 stream. */
int tw_np_randint_batch(uint32_t* key, int32_t* pos, int32_t n_calls, const int64_t* low,
                        const int64_t* high, const int64_t* cnt, int64_t* out);
/* tw_np_randint_batch narrowed to uint16, for calls on [0, high) with high <= 65536 (SWR_divide's
 * rows for the replay loop's narrowed row tables); 1 for any other call (state untouched). */
int tw_np_randint_batch_u16(uint32_t* key, int32_t* pos, int32_t n_calls, const int64_t* low,
                            const int64_t* high, const int64_t* cnt, uint16_t* out);
int tw_np_mt_next32(uint32_t* key, int32_t* pos, int64_t cnt, uint32_t* out);
/* grad_inc_block's draws for every shard of one UN_split call: for s < N, randint(0,kx,B)
 * into ix[s*B..] then randint(0,kz,B) into iz[s*B..].  Returns 1 if kx or kz <= 0. */
int tw_np_randint_pairs(uint32_t* key, int32_t* pos, int32_t N, int64_t kx, int64_t kz,
                        int64_t B, int64_t* ix, int64_t* iz);
/* S consecutive steps of those draws (the replay loop's segment between two reshuffles):
 * out is (S, 2, N, B) int64 — out[s][0] the step's X indices, out[s][1] its Z indices. */
int tw_np_randint_pairs_steps(uint32_t* key, int32_t* pos, int32_t S, int32_t N, int64_t kx,
                              int64_t kz, int64_t B, int64_t* out);
/* The same draws narrowed to uint16 (needs kx, kz <= 65536): a quarter of the bytes for the
 * replay loop's host-to-device copy; tw_widen_u16 restores the int64 indices on the device. */
int tw_np_randint_pairs_steps_u16(uint32_t* key, int32_t* pos, int32_t S, int32_t N,
                                  int64_t kx, int64_t kz, int64_t B, uint16_t* out);
/* The same draws narrowed to uint8 (needs kx, kz <= 256): half the bytes of the uint16 form. */
int tw_np_randint_pairs_steps_u8(uint32_t* key, int32_t* pos, int32_t S, int32_t N,
                                 int64_t kx, int64_t kz, int64_t B, uint8_t* out);
/* d_out[i] = d_in[i] (uint16 -> int64) for i < n, on `stream`; d_in may be the device address
 * of pinned host memory (tw_host_device_pointer): the kernel then reads it over PCIe, 16 B per
 * lane when d_in is 16-B aligned. */
int tw_widen_u16(const uint16_t* d_in, int64_t n, int64_t* d_out, void* stream);
/* The same for uint8 indices. */
int tw_widen_u8(const uint8_t* d_in, int64_t n, int64_t* d_out, void* stream);
/* The replay loop's segment upload in one launch: widen n narrowed draws (width 1 = uint8,
 * 2 = uint16) d_in -> d_out as above, and copy nx + nz 8-byte row indices d_rows ->
 * d_rows_x[0:nx], d_rows_z[0:nz] (a reshuffle's SWR tables; nx = nz = 0: none).  Either
 * source may be mapped host memory.  Replaces learning-experiment/make_exps.py:123-125's
 * SWR_divide hand-off + compute_stats.py:155-156's draws for one segment of steps. */
int tw_ship_draws(const void* d_in, int32_t width, int64_t n, int64_t* d_out,
                  const void* d_rows, int64_t nx, int64_t* d_rows_x, int64_t nz,
                  int64_t* d_rows_z, void* stream);
/* tw_ship_draws for a segment running through reshuffles: d_rows holds ntab tables, each
 * [nx x values | nz z values] of row_width bytes (8: int64, 2: uint16, widened), copied into
 * ntab consecutive tables of the stacks d_rows_x
 * (nx words apart) and d_rows_z (nz apart) — the input of tw_sgd_segment_narrow_tables. */
int tw_ship_draws_tables(const void* d_in, int32_t width, int64_t n, int64_t* d_out,
                         const void* d_rows, int32_t row_width, int32_t ntab, int64_t nx,
                         int64_t* d_rows_x, int64_t nz, int64_t* d_rows_z, void* stream);
/* The replay loop's draws made ahead on a native thread (csrc/drawpipe.hip): segment j of
 * n_seg (seg_steps[j] steps, its first step being step seg_phase[j] of a reshuffle period of
 * `mod` steps: a reshuffle before each of its steps k with (seg_phase[j] + k) % mod == 0) is
 * drawn from NumPy's MT19937 state (key/pos, advanced in place) into ring buffer j % nbuf, in
 * the reference's order: each reshuffle's SWR rows (make_exps.py:123-125,
 * compute_stats.py:48-54: N randint calls on [0, n_X) of n_X / N values, then N on [0, n_Z))
 * into the next of row_tabs tables of row_bufs[k] (N * (n_X/N + n_Z/N) values each, of
 * row_width bytes: 8 = int64, 2 = uint16 when n_X, n_Z <= 65536),
 * then the pairs (compute_stats.py:155-156) of the steps up to the next reshuffle into
 * seg_bufs[k] as (S, 2, N, B) values of `width` bytes (1, 2 or 8).  A segment with more
 * reshuffles than row_tabs fails the worker.  tw_draw_pipe_wait blocks until segment j is drawn; tw_draw_pipe_shipped records
 * that the uploads reading its buffers are enqueued on `stream` (the worker refills them only
 * after they have run); tw_draw_pipe_stop cancels what is not drawn, joins and frees.
 * Nothing else may use NumPy's global RNG between start and stop. */
int tw_draw_pipe_start(uint32_t* key, int32_t* pos, int32_t n_seg, const int32_t* seg_steps,
                       const int32_t* seg_phase, int64_t mod, int32_t N, int64_t kx, int64_t kz,
                       int64_t B, int64_t n_X, int64_t n_Z, int32_t width, int32_t nbuf,
                       void* const* seg_bufs, void* const* row_bufs, int32_t row_tabs,
                       int32_t row_width, void** out_handle);
int tw_draw_pipe_wait(void* handle, int32_t j);
int tw_draw_pipe_shipped(void* handle, int32_t j, void* stream);
int tw_draw_pipe_stop(void* handle);
/* n 8-byte words d_in -> d_out on `stream` (d_in may be mapped host memory, as above). */
int tw_copy_words(const void* d_in, int64_t n, void* d_out, void* stream);
/* learning_process's deferred evaluations (make_exps.py:143-190): one evaluation's nres
 * statistics, the nw words of w and (d_ctl not null) the SGD engine's abort word, written in one
 * launch into h_out, pinned host memory of nres + nw + 1 8-byte words. */
int tw_stage_eval(const void* d_res, int32_t nres, const void* d_w, int32_t nw,
                  const uint32_t* d_ctl, void* h_out, void* stream);
/* The call's final arrays over ranks by ONE exchange (round 6): tw_chain_final_pack packs this
 * rank's walked elements — scores d_x / d_z, rank-image records d_x_rec / d_z_rec, final global
 * positions d_x_pos / d_z_pos (the chains' state after the call's last emission), n_x / n_z a
 * rank — into world buckets of 1 + cap 24-B records {score, record, local position; z: n_x +
 * position} (d_send: world * (cap + 1) * 3 u64; d_cursor: world u64, zero on entry, left
 * zero); after an equal-split all-to-all tw_chain_final_scatter writes every received record
 * at its position of d_x_out / d_x_rec_out / d_z_out / d_z_rec_out (n_x / n_z 8-B words).
 * est.UnNT's final in-place arrays (main.py:46-47) over ranks.  Overflows raise *d_flag. */
int tw_chain_final_pack(const void* d_x, const uint64_t* d_x_rec, const uint32_t* d_x_pos,
                        int64_t n_x, const void* d_z, const uint64_t* d_z_rec,
                        const uint32_t* d_z_pos, int64_t n_z, int32_t world, int64_t cap,
                        uint64_t* d_cursor, void* d_send, int32_t* d_flag, void* stream);
int tw_chain_final_scatter(const void* d_recv, int32_t world, int64_t cap, int64_t n_x,
                           int64_t n_z, void* d_x_out, void* d_x_rec_out, void* d_z_out,
                           void* d_z_rec_out, int32_t* d_flag, void* stream);
/* A chunk's receive side over ranks in ONE call (round 6): tw_chain_unpack (its arguments, in
 * order) then tw_count_pairs_chain on the filled bags (shard offsets d_x_off / d_z_off, largest
 * shards max_nx / max_nz, bag strides n_x / n_z, out [steps][n_shards]), the cursors and the
 * counts zeroed by one launch — est.UnNT's per-step counts (main.py:72-79) of a chunk. */
int tw_chain_unpack_count(const uint64_t* d_recv, int32_t world, int32_t steps, int64_t cap,
                          int32_t half, int64_t n_x, int64_t n_z, int64_t x_shard,
                          int64_t z_shard, int32_t n_shards, void* d_x_bag, void* d_z_bag,
                          uint32_t* d_cursors, int32_t* d_flag, const int64_t* d_x_off,
                          const int64_t* d_z_off, int64_t max_nx, int64_t max_nz,
                          uint64_t* d_out, void* stream);
/* tw_chain_unpack_count whose count is tw_count_pairs_chain_planes' (image_bound: its promise;
 * d_work, work_bytes: its workspace, for bag strides n_x / n_z). */
int tw_chain_unpack_count_planes(const uint64_t* d_recv, int32_t world, int32_t steps,
                                 int64_t cap, int32_t half, int64_t n_x, int64_t n_z,
                                 int64_t x_shard, int64_t z_shard, int32_t n_shards,
                                 void* d_x_bag, void* d_z_bag, uint32_t* d_cursors,
                                 int32_t* d_flag, const int64_t* d_x_off,
                                 const int64_t* d_z_off, int64_t max_nx, int64_t max_nz,
                                 int64_t image_bound, uint64_t* d_out, void* stream,
                                 void* d_work, int64_t work_bytes);
/* The incomplete statistic on the step chains over ranks (cs.UnNBT, compute_stats.py:119-123,
 * with device-RNG draws): tw_chain_unpack_exact writes every received record {image, local
 * position} of a chunk's (source, step) buckets (tw_chain_emit's exchange layout, strict
 * images) at its exact position of the step's bags [steps][n_x] / [steps][n_z];
 * tw_count_pairs_chain_rng counts B device-drawn pairs (tw_count_pairs_rng's Philox/Lemire
 * draws, step c keyed seed + c, shard streams stream_id + s) of every (step, shard) bag on
 * those images, out [steps][n_shards] (zeroed here). */
int tw_chain_unpack_exact(const uint64_t* d_recv, int32_t world, int32_t steps, int64_t cap,
                          int64_t n_x, int64_t n_z, void* d_x_bag, void* d_z_bag,
                          int32_t* d_flag, void* stream);
int tw_count_pairs_chain_rng(const float* d_x_bag, const int64_t* d_x_off, int64_t x_stride,
                             const float* d_z_bag, const int64_t* d_z_off, int64_t z_stride,
                             int32_t n_shards, int32_t steps, int64_t max_nx, int64_t max_nz,
                             int64_t B, uint64_t seed, uint64_t stream_id, uint64_t* d_out,
                             void* stream);
/* The carried rank images' validity check (ShardedSample.UnN_many, device.py CARRY_IMAGES;
 * the arrays only ever permute between calls, estimation-experiment/main.py:43-44): *d_acc =
 * sum over the na + nb 8-byte words of [d_a | d_b] of a position-keyed 64-bit hash (d_acc:
 * tw_words_checksum_acc_words() u64 words, the rest scratch for the blocks' partials).  With
 * d_expect (one device word) and d_verdict (one int64; device or mapped host memory) both set,
 * also *d_verdict = (*d_acc == *d_expect) ? good : bad, in stream order. */
int tw_words_checksum(const void* d_a, int64_t na, const void* d_b, int64_t nb, void* d_acc,
                      const void* d_expect, void* d_verdict, int64_t good, int64_t bad,
                      void* stream);
int64_t tw_words_checksum_acc_words(void);
/* The device address of pinned, mapped host memory (hipHostGetDevicePointer); TW_ERR_ARG when
 * `host` is not such memory. */
int tw_host_device_pointer(void* host, void** out_dev);
/* np.random.shuffle(x); np.random.shuffle(z) — the in-place shuffles of UN
 * (compute_stats.py:66-67, estimation-experiment/main.py:46-47) — on C-contiguous arrays of
 * nx / nz items of isx / isz bytes (rows of a 2-D array are items): legacy RandomState's
 * _shuffle_raw restated (i = n-1 down to 1: j = masked-rejection draw on [0, i], swap), the same
 * draws from the same stream and the same final arrays; x's swaps run on a second thread while
 * z's draws and swaps run.  jbuf: nx + nz int64 of scratch.  Returns 2 on bad arguments. */
int tw_np_shuffle_pair(uint32_t* key, int32_t* pos, void* x, int64_t nx, int64_t isx, void* z,
                       int64_t nz, int64_t isz, int64_t* jbuf);
/* The index draws of np.random.shuffle on n <= 2^31 items WITHOUT the swaps (j[i] for
 * i = n-1 down to 1; j[0] untouched), advancing the state as the shuffle would: the host half
 * of the device shuffle below.  Returns 2 on bad arguments. */
int tw_np_shuffle_draws32(uint32_t* key, int32_t* pos, int64_t n, uint32_t* j);
/* The same draws for i = hi down to lo only (1 <= lo <= hi < n; j is the shuffle's n-entry
 * array, other entries untouched), the state advanced past them: consecutive ranges from
 * hi = n - 1 down to lo = 1 make exactly tw_np_shuffle_draws32's draws (the streamed last
 * shuffle of the drop-in).  Returns 2 on bad arguments. */
int tw_np_shuffle_draws32_range(uint32_t* key, int32_t* pos, int64_t n, int64_t hi, int64_t lo,
                                uint32_t* j);

/* ---- Device shuffle swaps (csrc/devshuffle.hip): the swaps of np.random.shuffle(x) and
 * np.random.shuffle(z) (UN's in-place shuffles, compute_stats.py:66-67,
 * estimation-experiment/main.py:46-47) on 8-byte items in HBM, from the host's draws
 * (tw_np_shuffle_draws32): for i = n-1 down to 1, swap a[i] and a[j[i]] — run as parallel
 * rounds with deterministic reservations, giving the sequential loop's permutation bit for bit.
 * One call enqueues tw_shuffle_swaps_rounds(nx, nz) rounds (first = 1, round0 = 0 on the first
 * call; later calls: first = 0, round0 += rounds) and writes the number of iterations still
 * pending to *d_pending (device u32); the caller repeats while it is non-zero (one call
 * suffices w.h.p.).  nx + nz < 2^31.  d_work: tw_shuffle_swaps_work_bytes bytes. */
int64_t tw_shuffle_swaps_work_bytes(int64_t nx, int64_t nz);
int32_t tw_shuffle_swaps_rounds(int64_t nx, int64_t nz);
/* rounds per batch (0 = the default 4.5 ln n + 24; at least 17): a test hook that forces resumed batches */
int tw_shuffle_swaps_set_rounds(int32_t rounds);
/* 1 (default): the tail rounds of a batch (every chunk entered, a short pending list) run in
 * one workgroup launch; 0: one launch per round.  Process-global; results do not depend on it. */
int tw_shuffle_swaps_set_tail(int32_t on);
int tw_shuffle_swaps(uint64_t* d_x, int64_t nx, uint64_t* d_z, int64_t nz, const uint32_t* d_jx,
                     const uint32_t* d_jz, int32_t first, int32_t round0, void* d_work,
                     uint32_t* d_pending, void* stream);
/* The draw windows of the rounds: iterations enter in W = tw_shuffle_swaps_windows() chunks of
 * p = ceil((n - 1) / W) draws, window c holding i in [max(1, n - (c + 1) p), n - c p). */
int32_t tw_shuffle_swaps_windows(void);
/* The first batch (first = 1, round0 = 0) of tw_shuffle_swaps enqueued in parts as the draws
 * arrive: rounds [r_begin, r_end) — round r reads windows 0 .. r + 1, so with windows [0, c)
 * on the device r_end = c - 1 (< W); r_begin = 0 also clears the workspace and reserves round
 * 0; last != 0 enqueues the remaining rounds, the tail and *d_pending (r_end ignored).  The
 * parts in sequence (each r_begin = the previous r_end) equal one tw_shuffle_swaps call. */
int tw_shuffle_swaps_part(uint64_t* d_x, int64_t nx, uint64_t* d_z, int64_t nz,
                          const uint32_t* d_jx, const uint32_t* d_jz, int32_t r_begin,
                          int32_t r_end, int32_t last, void* d_work, uint32_t* d_pending,
                          void* stream);

/* ---- MT19937 jump-ahead and NumPy-order randint streams on the device (csrc/mtjump.cpp host,
 * csrc/mtdraw.hip device).  The draws are those of consecutive legacy
 * np.random.randint(low, high, size) calls — cs.UB's two calls per block
 * (compute_stats.py:37-42) — made from NumPy's own MT19937 state without the indices crossing
 * PCIe: MT19937 is linear over GF(2), so the state J words ahead is a polynomial t^J mod phi in
 * the transition applied to the current state (Haramoto, Matsumoto, Nishimura, Panneton,
 * L'Ecuyer 2008), phi the degree-19937 minimal polynomial of the word recurrence (Matsumoto &
 * Nishimura 1998); for a fixed bound legacy randint is a masked rejection on consecutive
 * 32-bit words, i.e. a stream compaction of the raw words.
 * Polynomials are bit-packed in 312 uint64 (bit k = coefficient of t^k).
 * tw_mt_minpoly: phi (Berlekamp-Massey over GF(2), once per process).  tw_mt_jump_poly: t^J mod
 * phi, J >= 0.  tw_mt_poly_mulmod: a * b mod phi (reduced operands; out may alias).
 * tw_mt_jump_host: a NumPy (key[624], pos) state advanced by exactly J words, in NumPy's
 * representation (what J genrand_int32 calls leave).  Host entries return 0, 1 on bad arguments,
 * 2 if phi could not be found. */
int tw_mt_minpoly(uint64_t* out);
int tw_mt_jump_poly(int64_t J, uint64_t* out);
int tw_mt_poly_mulmod(const uint64_t* a, const uint64_t* b, uint64_t* out);
int tw_mt_jump_host(uint32_t* key, int32_t* pos, int64_t J);
/* Sub-stream states by doubling.  With x[i] the raw word sequence aligned to the host state
 * (x[0..623] = key) and L = 624 * stream_blocks, d_table[n_states][624] receives row 0 = key and
 * row k >= 1 = x[kL - 1 .. kL + 622] (the window one word BEFORE the sub-stream: its word 0
 * carries only the top bit, and x[kL + 623] follows by one recurrence step — the low 31 bits of a
 * window's word 0 are not state).  Level v makes rows [2^v, 2^(v+1)) from rows [0, 2^v), one
 * workgroup per row: d_polys[levels][2][19968] holds t^(2^v L - 1) (applied to row 0) and
 * t^(2^v L) (applied to the others), each as the LIST of its set coefficients: word 0 = the
 * number of listed positions (a multiple of 16, <= 19952), words 16.. = the positions, padded
 * with 20560 (a zero word of the kernel's sequence); levels >= ceil(log2 n_states). */
int tw_mt_states(const uint32_t* key, int32_t n_states, const uint32_t* d_polys, int32_t levels,
                 uint32_t* d_table, void* stream);
/* The tempered words x[0 .. n_states * L) of a state table into d_words, and for each of the
 * n_cfg <= 4 (mask, range) configurations the number of words of every key block (624 words)
 * with (w & mask) <= range into d_counts[n_cfg][n_states * stream_blocks]. */
int tw_mt_generate(const uint32_t* d_table, int32_t n_states, int32_t stream_blocks,
                   int32_t n_cfg, const uint32_t* cfg_mask, const uint32_t* cfg_rng,
                   uint32_t* d_words, uint32_t* d_counts, void* stream);
/* One round of n_calls consecutive masked-rejection randint calls on the words of a state table
 * made from (key, *pos): call c draws call_cnt[c] values v = w & cfg_mask[f] <= cfg_rng[f],
 * f = call_cfg[c], from the words that follow call c - 1's last one (the first call starts at
 * word *pos), and writes int32 call_base[c] + v at d_out[call_out[c] ...] (d_out: out_len
 * entries).  progress[0..2] = calls completed, values written of the first incomplete call,
 * words consumed; (key, *pos) is advanced past the consumed words in NumPy's representation.
 * A round whose words run out leaves the rest to the next round (a fresh table from the new
 * state).  Synchronises the stream.  d_work: tw_np_randint_dev_work_bytes bytes. */
int64_t tw_np_randint_dev_work_bytes(int32_t n_states, int32_t stream_blocks, int32_t n_calls,
                                     int32_t n_cfg);
int tw_np_randint_dev(uint32_t* key, int32_t* pos, const uint32_t* d_table, int32_t n_states,
                      int32_t stream_blocks, int32_t n_calls, const int32_t* call_cfg,
                      const int64_t* call_cnt, const int32_t* call_base, const int64_t* call_out,
                      int32_t n_cfg, const uint32_t* cfg_mask, const uint32_t* cfg_rng,
                      int32_t* d_out, int64_t out_len, void* d_work, int64_t* progress,
                      void* stream);

/* ---- One-sample pairwise U-statistics (csrc/selfpairs.hip; tuplewise.onesample; DESIGN.md
 * §4.9; an extension, not in the reference).  Pairs i < j of ONE sample, per shard:
 *   TW_SELF_GINI     sum |s_i - s_j|                          one double
 *   TW_SELF_VAR      sum (s_i - s_j)^2 / 2                    one double
 *   TW_SELF_KENDALL  items (a, b) of two 8-byte values; five uint64 C, D, Tx, Ty, Txy:
 *                    C = #{(a_i>a_j & b_i>b_j) | (a_i<a_j & b_i<b_j)}, D = the two mixed cases,
 *                    Tx = #{a_i==a_j}, Ty = #{b_i==b_j}, Txy = #{both} — plain comparisons of
 *                    the raw values (NaN compares false, -0.0 == 0.0; TW_I64 as int64).
 * d_off[n_shards + 1] counts items; shards of any mix of sizes run in one launch, a shard of
 * fewer than 2 items gives zeros.  The float kernels take TW_F64 only.  tw_self_pairs walks the
 * triangle of tile pairs (tw_self_pairs_tile() points per tile edge), each unordered pair once;
 * tw_self_pairs_idx32 evaluates pairs (d_i[p], d_j[p]), absolute item positions, for p in
 * [d_pair_off[s], d_pair_off[s + 1]).  Results do not depend on scheduling: block partials go
 * through d_work (tw_self_pairs_work_bytes / tw_self_pairs_idx_work_bytes bytes) and are added
 * in a fixed order.  Argument errors (n_shards < 0, a negative size, an unknown kern or dtype,
 * a float kern with TW_I64) return TW_ERR_ARG before any device work. */
#define TW_SELF_GINI 0
#define TW_SELF_VAR 1
#define TW_SELF_KENDALL 2
int64_t tw_self_pairs_work_bytes(int32_t n_shards, int64_t max_n);
int64_t tw_self_pairs_idx_work_bytes(int32_t n_shards, int64_t max_pairs);
int32_t tw_self_pairs_tile(void);
int tw_self_pairs(const void* d_s, const int64_t* d_off, int32_t n_shards, int64_t max_n,
                  int32_t dtype, int32_t kern, void* d_work, void* d_out, void* stream);
int tw_self_pairs_idx32(const void* d_s, const int32_t* d_i, const int32_t* d_j,
                        const int64_t* d_pair_off, int32_t n_shards, int64_t max_pairs,
                        int32_t dtype, int32_t kern, void* d_work, void* d_out, void* stream);

/* ---- The same numbers for ONE large sample without walking its pairs (csrc/selfsorted.hip;
 * DESIGN.md §4.9b): chunk sorts and binary searches in every sorted chunk, O(n (n / chunk) log
 * chunk) per pass.  d_s, d_off, dtype and d_out are tw_self_pairs'; total_n >= d_off[n_shards] -
 * d_off[0] sizes the scratch, max_n <= 2^31 - 1 is the largest shard.
 *   TW_SELF_KENDALL  (TW_F64, TW_I64) the five uint64 C, D, Tx, Ty, Txy — exactly the integers of
 *                    tw_self_pairs on every input (NaN, -0.0, +-inf, INT64_MAX included): D is
 *                    the number of strict inversions of b over the points with no NaN sorted by
 *                    (a, b), C = v (v - 1) / 2 - Tx' - Ty' + Txy - D over those v points;
 *   TW_SELF_GINI     (TW_F64) sum_i (2 i - n + 1) s_(i) over the sorted shard: exact
 *                    two-products summed in double-double in a fixed order and rounded once, so
 *                    a shard's double has the same bits alone or beside other shards (it differs
 *                    from tw_self_pairs' blocked sum in the last bits).  NaN if the shard holds
 *                    a NaN, two +inf or two -inf, else +inf if it holds an infinity;
 *   TW_SELF_VAR      refused (TW_ERR_ARG): the variance is O(n) from the moments.
 * chunk: 0 for tw_self_sorted_chunk(), or a power of two in [1024, 16384] keys.  The Kendall
 * integers do not depend on it; the Gini double is summed in another order under another chunk
 * (each within an ulp of the exact sum).  The input is not modified; d_work holds
 * tw_self_sorted_work_bytes(...) bytes; everything is ordered on `stream`.  Argument errors
 * return TW_ERR_ARG before any launch. */
int64_t tw_self_sorted_work_bytes(int32_t n_shards, int64_t total_n, int64_t max_n, int32_t kern,
                                  int32_t chunk);
int32_t tw_self_sorted_chunk(void);
int tw_self_sorted(const void* d_s, const int64_t* d_off, int32_t n_shards, int64_t total_n,
                   int64_t max_n, int32_t dtype, int32_t kern, int32_t chunk, void* d_work,
                   void* d_out, void* stream);

/* ---- Kendall tau matrices over many columns (csrc/kendall.hip; tuplewise.kendall; DESIGN.md
 * §4.18; an extension, not in the reference).  With s_a(i, j) = sign(S[i, a] - S[j, a]) over the
 * rows of one shard,
 *     M[a, b] = sum_{i<j} s_a(i, j) s_b(i, j)      C - D of columns a and b (exact int64)
 *     U_a     = M[a, a]                            the pairs not tied in column a
 * so tau-a = M[a, b] / P and tau-b = M[a, b] / (sqrt(U_a) sqrt(U_b)).  Two steps:
 *
 * tw_col_ranks: d_s is row-major (rows, p) of TW_F64 or TW_I64, d_off[n_shards + 1] counts rows
 * as in tw_self_pairs (shards of any mix of sizes in one call).  Every column of every shard is
 * replaced by its strict-less ranks r_i = #{j in the shard : x_j < x_i}: equal values get equal
 * ranks and sign(r_i - r_j) = sign(x_i - x_j) (-0.0 ties with 0.0, +-inf are ordinary values,
 * TW_I64 is compared as int64; the input must hold no NaN).  The rank image d_ranks is
 * column-major per shard with no padding: shard s starts at element (d_off[s] - d_off[0]) p,
 * column c of it n_s elements after c n_s, total_n p elements in all.  width 16: uint16
 * elements holding r - 32768 as an int16 bit pattern (shards of at most 65536 rows); width 32:
 * int32.  tw_kendall_matrix_width(max_n) is the width tuplewise.kendall uses: 32 above 65536 rows,
 * else the hook's value, else 16.  The sorts work on chunks of tw_col_ranks_chunk(max_n) <= 16384
 * keys; d_work holds tw_col_ranks_work_bytes(...) bytes and needs no zeroing.
 *
 * tw_kendall_matrix: two rank images of the SAME shards (d_off, width), columns A (pa) and B
 * (pb), each 1..1024; the same pointer and pa == pb is the symmetric call.  Per shard d_m holds
 * pa x pb int64 (row-major), d_ua pa and d_ub pb int64; a shard of fewer than 2 rows gives zeros.
 * Columns run in groups of 64, all group pairs in one launch; the symmetric call computes the
 * group pairs ga <= gb and the upper 16 x 16 blocks only and mirrors them, so M == M^T exactly
 * and Ua == Ub == diag(M).  Work items are the tile pairs of the triangle of
 * tw_kendall_matrix_tile() rows per tile edge, each unordered pair of rows once.  The integers
 * do not depend on scheduling (integer atomics); the caller zeroes nothing; d_work holds
 * tw_kendall_matrix_work_bytes(...) bytes.  Hooks (0 restores the default): _set_width(0 | 16 |
 * 32), _set_flush(k): the int32 accumulators are added to the int64 sums every k matrix
 * instructions as well as after every tile pair, _set_plan(max_wgs): at most max_wgs workgroups
 * per shard and group pair; each returns a status like every other entry, and all three are swept
 * at small shapes by tests/test_gpu_kendall_matrix.py.  Argument errors return TW_ERR_ARG before
 * any device work. */
int32_t tw_kendall_matrix_tile(void);
int32_t tw_kendall_matrix_width(int64_t max_n);
int32_t tw_col_ranks_chunk(int64_t max_n);
int32_t tw_kendall_matrix_set_width(int32_t width);
int32_t tw_kendall_matrix_set_flush(int32_t k);
int32_t tw_kendall_matrix_set_plan(int32_t max_wgs);
int64_t tw_col_ranks_work_bytes(int32_t n_shards, int64_t total_n, int64_t max_n, int32_t p);
int tw_col_ranks(const void* d_s, const int64_t* d_off, int32_t n_shards, int64_t total_n,
                 int64_t max_n, int32_t p, int32_t dtype, int32_t width, void* d_work,
                 void* d_ranks, void* stream);
int64_t tw_kendall_matrix_work_bytes(int32_t n_shards, int32_t pa, int32_t pb);
int tw_kendall_matrix(const void* d_ra, int32_t pa, const void* d_rb, int32_t pb,
                      const int64_t* d_off, int32_t n_shards, int64_t max_n, int32_t width,
                      void* d_work, int64_t* d_m, int64_t* d_ua, int64_t* d_ub, void* stream);

/* ---- The per-point row sums behind the variance of a Kendall tau matrix (csrc/kendall_rows.hip;
 * tuplewise.kendall_var; an extension).  With the signs above and, for a point i
 * of a shard,
 *     c_i(a, b) = sum over j != i of s_a(i, j) s_b(i, j)      |c_i| <= n_s - 1
 *     u_i(a)    = c_i(a, a)                                   the points not tied with i in a
 * tw_kendall_rows takes ONE rank image of tw_col_ranks (d_ranks, p columns, d_off, width as
 * tw_kendall_matrix takes them: the symmetric case only) and writes four (n_shards, p, p) int64
 * arrays, row-major:
 *     d_r[a, b] = sum_i c_i(a, b)              (= 2 M[a, b] of tw_kendall_matrix; d_r[a, a] = 2 U_a)
 *     d_q[a, b] = sum_i c_i(a, b)^2
 *     d_f[a, b] = sum_i c_i(a, b) u_i(a)       (not symmetric)
 *     d_e[a, b] = sum_i u_i(a) u_i(b)
 * d_r, d_q and d_e equal their transposes exactly.  A shard of fewer than 2 rows gives zeros.
 * max_n <= 2^20 keeps every sum below 2^63.  Work items are runs of anchors i per shard and pair of
 * 64-column groups, every anchor against all points of its shard; the integers do not depend on
 * scheduling or on the hooks (integer atomics); the caller zeroes nothing; d_work holds
 * tw_kendall_rows_work_bytes(n_shards, p) bytes (0 for sizes tw_kendall_rows refuses).  The
 * diagonal groups, a partly filled last group and the pairs of groups go out as separate kernel
 * launches, each planned by itself.  Hooks: _set_plan(max_wgs): at most max_wgs workgroups per
 * shard and work item; _set_anchors(k): a wave carries at most k = 1, 2 or 4 anchors at once — a
 * kernel shape whose registers do not hold k runs fewer without saying so (the hook keeps
 * reporting k): 2 instead of 4 between two groups and at 4 column blocks of int32 ranks, and 1
 * for the pairs with a partly filled last group in int32; the plan is sized by the anchors that
 * run; 0 restores the default.  A hook returns the value it replaced, or -1 for a value it refuses (tw_last_error
 * says why); both are swept by tests/test_gpu_kendall_rows.py.  Argument errors (a null buffer,
 * n_shards < 0, p outside [1, 1024], max_n outside [0, 2^20], a width other than 16 or 32, a
 * 16-bit image of more than 65536 rows) return TW_ERR_ARG before any launch. */
int32_t tw_kendall_rows_set_plan(int32_t max_wgs);
int32_t tw_kendall_rows_set_anchors(int32_t k);
int64_t tw_kendall_rows_work_bytes(int32_t n_shards, int32_t p);
int tw_kendall_rows(const void* d_ranks, int32_t p, const int64_t* d_off, int32_t n_shards,
                    int64_t max_n, int32_t width, void* d_work, int64_t* d_r, int64_t* d_q,
                    int64_t* d_f, int64_t* d_e, void* stream);

/* ---- Two-sample triplet U-statistics of degree (2,1) (csrc/triplets.hip; tuplewise.triplets;
 * DESIGN.md §4.10; an extension, not in the reference): h = 1{D(x_i, z_k) > D(x_i, x_j)}, j != i,
 * for an anchor x_i, a point x_j of its own class and a point z_k of the other class.  d_x is
 * (rows, d) and d_z (rows, d) float64, row-major, 1 <= d <= 64.  D(a, b) is the squared
 * Euclidean distance in ONE arithmetic order, multiply and add separate (never fused):
 *   acc = 0.0; for c = 0 .. d-1: t = a_c - b_c; acc = acc + t * t
 * so a distance has the same bits wherever it is computed; a NaN distance is
 * written as the quiet NaN 0x7ff8000000000000, whichever NaN the arithmetic returned.
 *
 * tw_triplet_rows writes, for every anchor a in [a_begin, a_end) (absolute rows of d_x), the two
 * rows whose two-sample count is the anchor's triplet count.  The partition is given by block
 * offsets: block b owns rows [d_blk_x_off[b], d_blk_x_off[b + 1]) of d_x (n_b of them) and rows
 * [d_blk_z_off[b], d_blk_z_off[b + 1]) of d_z (m_b); an anchor is compared with its own block
 * only.  blk_first / blk_count name the blocks the anchor range touches (naming more is
 * harmless), max_n / max_m bound their n_b / m_b.  With q = a - a_begin:
 *   "other" row  d_other[d_other_off[q] + k]  = D(x_a, z_k), k = 0 .. m_b - 1 (block-relative)
 *   "own" row    d_own[d_own_off[q] + j']     = D(x_a, x_j), j != a, j' = j for j < a and j - 1
 *                                               for j > a (block-relative): n_b - 1 entries
 * The caller sizes d_other / d_own and packs the rows back to back, so that d_other_off /
 * d_own_off (a_end - a_begin + 1 entries) are the d_x_off / d_z_off of tw_count_pairs or
 * tw_count_pairs_sorted with one anchor per shard.  Blocks of any mix of sizes share the launch;
 * no atomics, nothing to zero.  tw_triplet_rows_tile(): points per tile edge of the kernel.
 *
 * tw_triplet_idx32 counts given triplets: for p in [d_trip_off[s], d_trip_off[s + 1]), rows
 * d_i[p], d_j[p] of d_x and d_k[p] of d_z (absolute, int32); d_out[s] (uint64) =
 * #{D(x_i, z_k) > D(x_i, x_j)} for TW_PRED_GT, 2 #{>} + #{==} for TW_PRED_HALF (IEEE compares: a
 * NaN distance counts for neither).  Block partials go through d_work
 * (tw_triplet_idx_work_bytes bytes) and are added in a fixed order, as tw_self_pairs_idx32's.
 *
 * Argument errors (a null pointer, d outside [1, 64], a negative size, an empty anchor range,
 * another predicate) return TW_ERR_ARG before any device work. */
int32_t tw_triplet_rows_tile(void);
int tw_triplet_rows(const double* d_x, const double* d_z, int32_t d, const int64_t* d_blk_x_off,
                    const int64_t* d_blk_z_off, int32_t blk_first, int32_t blk_count,
                    int64_t a_begin, int64_t a_end, int64_t max_n, int64_t max_m,
                    const int64_t* d_other_off, const int64_t* d_own_off, double* d_other,
                    double* d_own, void* stream);
int64_t tw_triplet_idx_work_bytes(int32_t n_shards, int64_t max_triplets);
int tw_triplet_idx32(const double* d_x, const double* d_z, int32_t d, const int32_t* d_i,
                     const int32_t* d_j, const int32_t* d_k, const int64_t* d_trip_off,
                     int32_t n_shards, int64_t max_triplets, int32_t pred, void* d_work,
                     uint64_t* d_out, void* stream);

/* ---- Triplet metric learning (csrc/triplet_grad.hip; tuplewise.triplet_learning; DESIGN.md
 * §4.11; an extension, not in the reference): a linear map d_L (p, d) float64 row-major,
 * 1 <= p <= 64, on the samples of the section above (1 <= d <= 64), under the triplet hinge.  For
 * a triplet (i, j, k), a = x_i - x_j, b = x_i - z_k, u = L a, v = L b:
 *   S = margin + |u|^2 - |v|^2,   loss = max(S, 0),   G_t = 1{S > 0} * 2 (u a^T - v b^T)
 *
 * tw_triplet_grad takes triplets as tw_triplet_idx32 does (absolute int32 rows, shard s owns
 * [d_trip_off[s], d_trip_off[s + 1]), any mix of sizes, max_triplets bounds them) and writes
 *   d_loss[s]   the shard's mean loss (an empty shard: 0)              n_shards doubles
 *   d_active[s] #{S > 0} of the shard                                  n_shards uint64
 *   d_G         the mean over non-empty shards of the shards' mean G_t (p, d), all zero when
 *               every shard is empty; left untouched (and may be null) when want_grad = 0
 * d_loss and d_active are always written.  G and the loss carry no bit contract (fused
 * multiply-adds, sums in the kernel's order) but are run-to-run deterministic: no atomics, one
 * partial per workgroup in d_work (tw_triplet_grad_work_bytes bytes, nothing to zero), added in
 * workgroup order, then the shards' means in a fixed order that no schedule changes.
 * tw_triplet_grad_tile(): triplets per workgroup.
 *
 * tw_triplet_project: d_out[row * p + r] = acc over c = 0 .. d-1 of acc + L[r, c] * A[row, c]
 * from acc = 0.0, multiply and add separate — bit-exact; a NaN is written as the quiet NaN
 * 0x7ff8000000000000.  d_a is (rows, d).
 *
 * tw_triplet_sgd_update, over count = p * d elements, multiply and add separate (bit-exact given
 * d_G): g = G + reg * L; delta = lr * g (momentum = 0) or 0.9 * delta + lr * g (momentum = 1);
 * L = L - delta.  d_L and d_delta are updated in place.
 *
 * Argument errors (a null pointer, d or p outside [1, 64], a negative size, want_grad or
 * momentum not 0 / 1, a NaN margin) return TW_ERR_ARG before any launch. */
int32_t tw_triplet_grad_tile(void);
int64_t tw_triplet_grad_work_bytes(int32_t n_shards, int64_t max_triplets, int32_t d, int32_t p);
int tw_triplet_grad(const double* d_x, const double* d_z, int32_t d, const double* d_L, int32_t p,
                    const int32_t* d_i, const int32_t* d_j, const int32_t* d_k,
                    const int64_t* d_trip_off, int32_t n_shards, int64_t max_triplets,
                    double margin, int32_t want_grad, void* d_work, double* d_G, double* d_loss,
                    uint64_t* d_active, void* stream);
int tw_triplet_project(const double* d_a, int64_t rows, int32_t d, const double* d_L, int32_t p,
                       double* d_out, void* stream);
int tw_triplet_sgd_update(const double* d_G, double* d_L, double* d_delta, int32_t count,
                          double reg, double lr, int32_t momentum, void* stream);

/* ---- Kernel two-sample U-statistics of degree (2,2) (csrc/mmd.hip; tuplewise.mmd; DESIGN.md
 * §4.12; an extension, not in the reference): the unbiased squared maximum mean discrepancy and
 * the energy distance, both the mean over quadruples of
 *   h((x, x'), (z, z')) = g(x, x') + g(z, z') - g(x, z') - g(x', z)
 * d_x is (rows, d) and d_z (rows, d) float64, row-major, 1 <= d <= 64.  D(a, b) is the squared
 * Euclidean distance of the triplet section, in the same arithmetic order and by the same device
 * functions (csrc/tripdist.h): acc = 0.0; for c = 0 .. d-1: t = a_c - b_c; acc = acc + t * t,
 * multiply and add separate, direct differences only — so D(a, a) = 0 exactly and D(a, b) =
 * D(b, a) bit for bit.  The pair function g:
 *   TW_MMD_GAUSSIAN  g = exp(fl(c * D)), the float64 exp of the device library; c = -1 / (2
 *                    sigma^2) is computed by the caller and must be finite and <= 0
 *   TW_MMD_ENERGY    g = sqrt(D), the correctly rounded float64 square root; c is ignored
 *
 * tw_mmd_sums reduces on the device: the partition is given as tw_triplet_rows takes it (block b
 * owns rows [d_blk_x_off[b], d_blk_x_off[b + 1]) of d_x and [d_blk_z_off[b], d_blk_z_off[b + 1])
 * of d_z, absolute offsets, n_blocks + 1 entries each; max_n / max_m bound the blocks' sizes),
 * blocks of any mix of sizes share one launch, and for every block three doubles are written:
 *   d_out[3 b + 0] = Sxx = sum over i < j of g(x_i, x_j)
 *   d_out[3 b + 1] = Szz = sum over k < l of g(z_k, z_l)
 *   d_out[3 b + 2] = Sxz = sum over all (i, k) of g(x_i, z_k)
 * each unordered pair visited once (the triangles of tile pairs, tw_mmd_tile() rows per tile
 * edge, and the rectangle of X tiles by Z tiles); a block of fewer than 2 rows of a sample has a
 * zero sum there.  The statistic is the caller's: V = 2 Sxx / (n (n - 1)) + 2 Szz / (m (m - 1)) -
 * 2 Sxz / (n m), MMD^2_u = V for the Gaussian kernel and the energy distance = -V.
 *
 * tw_mmd_idx32 evaluates given quadruples: for p in [d_quad_off[s], d_quad_off[s + 1]), rows
 * d_i[p], d_j[p] of d_x and d_k[p], d_l[p] of d_z (absolute, int32), four doubles per shard:
 *   d_out[4 s + 0] = sum g(x_i, x_j)    d_out[4 s + 1] = sum g(z_k, z_l)
 *   d_out[4 s + 2] = sum g(x_i, z_l)    d_out[4 s + 3] = sum g(x_j, z_k)
 * an empty shard gives zeros.
 *
 * The sums carry no bit contract (floats added in the kernel's order), but they are run-to-run
 * deterministic and a block's (shard's) doubles are the same bits alone in a launch or beside
 * others: no atomics, one partial per workgroup in d_work (tw_mmd_work_bytes /
 * tw_mmd_idx_work_bytes bytes, nothing to zero), added in a fixed order as tw_self_pairs'.  A NaN
 * coordinate makes every sum it enters NaN; infinities follow IEEE arithmetic.
 *
 * Argument errors (a null pointer, d outside [1, 64], a negative size, an unknown kernel id, a
 * non-finite or positive c for the Gaussian kernel) return TW_ERR_ARG before any device work. */
#define TW_MMD_GAUSSIAN 0
#define TW_MMD_ENERGY 1
int32_t tw_mmd_tile(void);
int64_t tw_mmd_work_bytes(int32_t n_blocks, int64_t max_n, int64_t max_m);
int64_t tw_mmd_idx_work_bytes(int32_t n_shards, int64_t max_quads);
int tw_mmd_sums(const double* d_x, const double* d_z, int32_t d, const int64_t* d_blk_x_off,
                const int64_t* d_blk_z_off, int32_t n_blocks, int64_t max_n, int64_t max_m,
                int32_t kern, double c, void* d_work, double* d_out, void* stream);
int tw_mmd_idx32(const double* d_x, const double* d_z, int32_t d, const int32_t* d_i,
                 const int32_t* d_j, const int32_t* d_k, const int32_t* d_l,
                 const int64_t* d_quad_off, int32_t n_shards, int64_t max_quads, int32_t kern,
                 double c, void* d_work, double* d_out, void* stream);

/* ---- The permutation test of the statistics above (csrc/mmd_perm.hip; tuplewise.mmd
 * permutation_sums / permutation_test; an extension): Sxx, Szz, Sxz of EVERY
 * relabelling of the pooled sample in one launch.  d_w is the pooled sample, (n_rows, d) float64
 * row-major, first sample first; g, kern and c as above.  d_labels[r * W + w], W = ceil(n_perm /
 * 32) uint32 words a row: bit b is 1 iff row r is in the first sample under permutation
 * (column) 32 w + b; padding bits are 0.  For every column p
 *   d_out[3 p + 0] = Sxx_p   d_out[3 p + 1] = Szz_p   d_out[3 p + 2] = Sxz_p
 * as tw_mmd_sums orders them.  Each g(w_i, w_j), i < j, is evaluated once per pass of
 * tw_mmd_perm_cols() columns and multiplied by the labels as exact 0.0 / 1.0 on the float64
 * matrix unit: with s the column's labels, Sxx = sum s_i s_j g_ij, A = sum (s_i + s_j) g_ij,
 * T = sum g_ij, Sxz = A - 2 Sxx and Szz = T - A + Sxx (Szz and Sxz are differences of sums of
 * the size of T).  No atomics: one partial per workgroup and column in d_work
 * (tw_mmd_perm_work_bytes bytes, nothing to zero), added in a fixed order.  Results are run-to-run
 * deterministic, and a column's three doubles depend only on d_w and on that column's labels —
 * not on its position p, on n_perm or on the other columns.  A NaN coordinate anywhere makes
 * every column NaN (0 * NaN).
 *
 * TW_ERR_ARG before any device work: a null pointer, d outside [1, 64], n_rows < 4 or >= 2^31,
 * n_perm < 1 (a test has at least the observed split), an unknown kernel id, a non-finite or
 * positive c for the Gaussian kernel, a grid past 2^31 workgroups.  tw_mmd_perm_work_bytes is 0
 * for sizes tw_mmd_perm_sums refuses. */
int32_t tw_mmd_perm_cols(void);
int64_t tw_mmd_perm_work_bytes(int64_t n_rows, int32_t n_perm);
int tw_mmd_perm_sums(const double* d_w, int64_t n_rows, int32_t d, const uint32_t* d_labels,
                     int32_t n_perm, int32_t kern, double c, void* d_work, double* d_out,
                     void* stream);

/* ---- The row sums of the statistics above, for a grid of bandwidths (csrc/mmd_rows.hip;
 * tuplewise.mmd_var; an extension): the partition, d, D, g and kern are
 * tw_mmd_sums'; d_c holds n_sigma coefficients c_s = -1 / (2 sigma_s^2) in DEVICE memory (under
 * TW_MMD_ENERGY n_sigma is 1 and d_c is not read).  With nx = d_blk_x_off[n_blocks] and nz =
 * d_blk_z_off[n_blocks] the rows the offsets span, every row i of X and k of Z that belongs to a
 * block gets, for every s,
 *   d_rows_x[(s * nx + i) * 2 + 0] = sum over j != i of the block's X of g_s(x_i, x_j)
 *   d_rows_x[(s * nx + i) * 2 + 1] = sum over k of the block's Z of g_s(x_i, z_k)
 *   d_rows_z[(s * nz + k) * 2 + 0] = sum over i of the block's X of g_s(x_i, z_k)
 *   d_rows_z[(s * nz + k) * 2 + 1] = sum over l != k of the block's Z of g_s(z_k, z_l)
 * (absolute rows; rows before the first block are not written; a block of fewer than 2 rows of a
 * sample has zeros in the sums over that sample's pairs).  Each unordered pair is visited once:
 * D is evaluated once per pair and g applied n_sigma times to the held D, so a term has the bits
 * tw_mmd_sums gives it, exp(fl(c_s * D)).  A pair feeds its point's sum in a register and its
 * anchor's through a cross-lane reduce-scatter; one partial per row, tile column and sigma goes to
 * d_work (tw_mmd_rows_work_bytes bytes, nothing to zero) and a second kernel adds a row's
 * partials in a fixed order of the columns.  No atomics; results are run-to-run deterministic, a
 * block's rows are the same bits alone, beside other blocks and wherever the partition starts,
 * and a sigma's rows do not depend on n_sigma, on its position s or on the other coefficients.
 * The coefficients live on the device, so TW_MMD_KERN_CHECKS' test of c is the caller's.
 *
 * TW_ERR_ARG before any device work: a null pointer (d_c may be null for the energy kernel), d
 * outside [1, 64], an unknown kernel id, n_sigma outside [1, tw_mmd_rows_max_sigma()] or != 1 for
 * the energy kernel, a negative size, max_n or max_m >= 2^31, a grid past 2^31 workgroups,
 * d_work past 1 GiB.  tw_mmd_rows_work_bytes is 0 for shapes tw_mmd_rows refuses. */
int32_t tw_mmd_rows_max_sigma(void);
int64_t tw_mmd_rows_work_bytes(int32_t n_blocks, int64_t max_n, int64_t max_m, int32_t n_sigma);
int tw_mmd_rows(const double* d_x, const double* d_z, int32_t d, const int64_t* d_blk_x_off,
                const int64_t* d_blk_z_off, int32_t n_blocks, int64_t max_n, int64_t max_m,
                int32_t kern, const double* d_c, int32_t n_sigma, void* d_work, double* d_rows_x,
                double* d_rows_z, void* stream);

/* ---- Kernel independence U-statistics of degree 4 on one paired sample (csrc/hsic.hip;
 * tuplewise.hsic; an extension): the unbiased Hilbert-Schmidt independence
 * criterion HSIC_u (Song et al. 2012) and the unbiased squared distance covariance
 * (Szekely-Rizzo 2014), with what their normalised forms need.  d_x is (rows, dx) and d_y
 * (rows, dy) float64, row-major, 1 <= dx, dy <= 64; row i of d_x and row i of d_y are one item.
 * D is the squared distance of the triplet section (csrc/tripdist.h) and g the pair function of
 * the MMD section (the same device functions, so a K_ij has the bits tw_mmd_sums gives it):
 *   K_ij = g(D(x_i, x_j); c_x)   L_ij = g(D(y_i, y_j); c_y)   zero diagonals
 *   TW_HSIC_GAUSSIAN  g = exp(fl(c * D)), c = -1 / (2 sigma^2) per side, finite and <= 0
 *   TW_HSIC_DISTANCE  g = sqrt(D); c_x, c_y are ignored
 * and the row sums k_i = sum over j != i of K_ij, l_i likewise.
 *
 * tw_hsic_sums: block b is rows [d_blk_off[b], d_blk_off[b + 1]) of BOTH arrays (absolute
 * offsets, n_blocks + 1 entries; max_n bounds the blocks' sizes and must be >= 4).  Blocks of any
 * mix of sizes share one launch, and for every block eight doubles are written:
 *   d_out[8 b + 0] = S_KL = sum over i < j of K_ij L_ij     d_out[8 b + 3] = R_K  = sum_i k_i
 *   d_out[8 b + 1] = S_KK = sum over i < j of K_ij K_ij     d_out[8 b + 4] = R_L  = sum_i l_i
 *   d_out[8 b + 2] = S_LL = sum over i < j of L_ij L_ij     d_out[8 b + 5] = R_KL = sum_i k_i l_i
 *   d_out[8 b + 6] = R_KK = sum_i k_i k_i                   d_out[8 b + 7] = R_LL = sum_i l_i l_i
 * If d_rows is not NULL, d_rows[2 i] = k_i and d_rows[2 i + 1] = l_i for every absolute row i
 * inside a block; rows outside every block are not written.  The statistic is the caller's (n the
 * block's rows): U(S, Ra, Rb, Rab) = (2 S + Ra Rb / ((n - 1)(n - 2)) - 2 Rab / (n - 2)) /
 * (n (n - 3)); HSIC_u or dCov^2_u = U(S_KL, R_K, R_L, R_KL), and the correlation divides by
 * sqrt(U(S_KK, R_K, R_K, R_KK) U(S_LL, R_L, R_L, R_LL)).
 *
 * Each unordered pair is evaluated once.  A workgroup owns a super-tile of group x group tiles
 * (tw_hsic_tile() rows per tile edge) of the triangle of super-tiles and leaves one row-sum
 * partial per row and super-tile column in d_work; `group` in [1, 8] is that launch-plan knob
 * (it changes which partials exist, so the last bits, never the contract), group = 0 chooses: the
 * largest group that leaves 1024 workgroups (1 if none does), raised while d_work would pass
 * 1 GiB.  tw_hsic_work_bytes is the size of d_work for the same arguments, 0 for shapes
 * tw_hsic_sums refuses (n_blocks < 1, max_n < 4, group outside [0, 8], d_work past 1 GiB, a grid
 * past 2^31 workgroups).
 *
 * tw_hsic_idx32 evaluates given 4-tuples: for p in [d_quad_off[s], d_quad_off[s + 1]), rows
 * i = d_i[p], j = d_j[p], q = d_q[p], r = d_r[p] (absolute, int32), three doubles per shard:
 *   d_out[3 s + 0] = A = sum K_ij L_ij   d_out[3 s + 1] = B = sum K_ij L_qr
 *   d_out[3 s + 2] = C = sum K_ij L_iq
 * (the mean of f = K_ij (L_ij + L_qr - 2 L_iq) is (A + B - 2 C) / count); an empty shard gives
 * zeros.  tw_hsic_idx_work_bytes is 0 for sizes tw_hsic_idx32 refuses.
 *
 * No bit contract on the sums (floats added in the kernel's order), but: no atomics, nothing to
 * zero, run-to-run deterministic, and a block's eight doubles and row sums (a shard's three) are
 * the same bits alone in a launch, beside others and wherever the partition starts.  Masked pairs
 * are selected away, so a NaN of another block never enters; a NaN coordinate of x makes the
 * K-derived outputs of its block NaN and leaves S_LL, R_L, R_LL and every l_i as they were.
 *
 * TW_ERR_ARG before any device work: a null pointer (d_rows may be NULL), dx or dy outside
 * [1, 64], a negative size, an unknown kernel id, a non-finite or positive c_x or c_y for the
 * Gaussian kernel, max_n < 4 (a block of fewer than 4 rows has no 4-tuple), group outside [0, 8],
 * d_work past its budget, a grid past 2^31 workgroups. */
#define TW_HSIC_GAUSSIAN 0
#define TW_HSIC_DISTANCE 1
int32_t tw_hsic_tile(void);
int64_t tw_hsic_work_bytes(int32_t n_blocks, int64_t max_n, int32_t group);
int64_t tw_hsic_idx_work_bytes(int32_t n_shards, int64_t max_quads);
int tw_hsic_sums(const double* d_x, int32_t dx, const double* d_y, int32_t dy,
                 const int64_t* d_blk_off, int32_t n_blocks, int64_t max_n, int32_t kern,
                 double c_x, double c_y, int32_t group, void* d_work, double* d_rows,
                 double* d_out, void* stream);
int tw_hsic_idx32(const double* d_x, int32_t dx, const double* d_y, int32_t dy,
                  const int32_t* d_i, const int32_t* d_j, const int32_t* d_q, const int32_t* d_r,
                  const int64_t* d_quad_off, int32_t n_shards, int64_t max_quads, int32_t kern,
                  double c_x, double c_y, void* d_work, double* d_out, void* stream);

/* ---- Three row sums per point of the independence statistics above, for a grid of bandwidth
 * pairs (csrc/hsic_rows.hip; tuplewise.hsic_var; an extension): what the
 * first-order variance of HSIC_u / dCov^2_u is estimated from.  The partition (d_blk_off, n_blocks,
 * max_n >= 4, blocks of any mix of sizes in one launch), dx, dy, D, g and kern are tw_hsic_sums',
 * and the step is its own (csrc/hsictile.h), so a K_ij or L_ij has the bits tw_hsic_sums gives it.
 * d_c holds n_sigma coefficient pairs in DEVICE memory, c_x[s] = d_c[2 s] and c_y[s] =
 * d_c[2 s + 1], each -1 / (2 sigma^2), with n_sigma in [1, tw_hsic_rows_max_sigma()]; under
 * TW_HSIC_DISTANCE n_sigma is 1 and d_c is not read.  With rows = d_blk_off[n_blocks] the rows
 * the offsets span, every absolute row i inside a block gets, for every s,
 *   d_rows[(s * rows + i) * 3 + 0] = sum over j != i of the block of K_ij L_ij
 *   d_rows[(s * rows + i) * 3 + 1] = sum over j of K_ij wk_j     (k_i where d_w is NULL)
 *   d_rows[(s * rows + i) * 3 + 2] = sum over j of L_ij wl_j     (l_i where d_w is NULL)
 * (rows outside every block are not written).  d_w is NULL (wk = wl = 1.0) or the d_rows of a
 * previous launch on the same partition and n_sigma, read at its stride of 3:
 *   wk_j = d_w[(s * rows + j) * 3 + 2]    wl_j = d_w[(s * rows + j) * 3 + 1]
 * and d_w[.. + 0] is not read.  So a first launch without weights gives (p, k, l) and a second one
 * with the first's d_rows as d_w gives (p, K l, L k); d_w and d_rows must not overlap.
 *
 * Each unordered pair is visited once: both squared distances are evaluated once per pair and g
 * is applied n_sigma times per side to the held values.  A pair feeds its point's sums in
 * registers and its anchor's through a cross-lane reduce-scatter; one partial per row, tile
 * column, sum and sigma goes to d_work (tw_hsic_rows_work_bytes bytes, nothing to zero) and a
 * second kernel adds a row's partials in a fixed order of the columns.  No atomics; results are
 * run-to-run deterministic, a block's rows are the same bits alone, beside other blocks and
 * wherever the partition starts, a pair's rows do not depend on n_sigma, on its position s or on
 * the other pairs, and [.. + 0] is the same bits with and without d_w.  Masked pairs (and their
 * weights) are selected away, so a NaN of another block never enters; a NaN coordinate of x makes
 * [.. + 0], [.. + 1] and, through a first launch's k as wl, the weighted [.. + 2] of its block
 * NaN and leaves the unweighted [.. + 2] = l_i as it was.  The coefficients live on the device,
 * so TW_HSIC_KERN_CHECKS' test of c (finite and <= 0) is the caller's.
 *
 * TW_ERR_ARG before any device work: a null pointer (d_w may be NULL; d_c may be NULL for the
 * distance kernel), dx or dy outside [1, 64], an unknown kernel id, n_sigma outside
 * [1, tw_hsic_rows_max_sigma()] or != 1 for the distance kernel, a negative size, max_n < 4 or
 * >= 2^31, a grid past 2^31 workgroups, d_work past 1 GiB.  tw_hsic_rows_work_bytes is 0 for
 * shapes tw_hsic_rows refuses (and for n_blocks < 1). */
int32_t tw_hsic_rows_max_sigma(void);
int64_t tw_hsic_rows_work_bytes(int32_t n_blocks, int64_t max_n, int32_t n_sigma);
int tw_hsic_rows(const double* d_x, int32_t dx, const double* d_y, int32_t dy,
                 const int64_t* d_blk_off, int32_t n_blocks, int64_t max_n, int32_t kern,
                 const double* d_c, int32_t n_sigma, const double* d_w, void* d_work,
                 double* d_rows, void* stream);

/* ---- The permutation test of the independence statistics above (csrc/hsic_perm.hip;
 * tuplewise.hsic_perm permutation_sums / permutation_test; an extension): the
 * two of tw_hsic_sums' eight sums that a permutation of the pairing moves, for EVERY permutation
 * in one launch.  One side is held and one is moved: d_held is (n, d_h) and d_moved (n, d_m) float64
 * row-major, H_ij = g(D(held_i, held_j); c_held) and M_ab = g(D(moved_a, moved_b); c_moved) with
 * D, g and kern (TW_HSIC_GAUSSIAN / TW_HSIC_DISTANCE) as above, so an H_ij has the bits
 * tw_hsic_sums gives it.  d_idx is (n_cols, n) int32 row-major: under column p item i pairs
 * held_i with moved_{idx[p][i]}.  d_rows_held and d_rows_moved are the n row sums of H and of M
 * on the unpermuted sample (tw_hsic_sums' d_rows, one side each).  For every column p
 *   d_out[2 p + 0] = S_p   = sum over i < j of H_ij M_{idx[p][i], idx[p][j]}
 *   d_out[2 p + 1] = Rab_p = sum over i of rows_held[i] rows_moved[idx[p][i]]
 * and HSIC_u (dCov^2_u) of the permuted pairing is U(S_p, R_held, R_moved, Rab_p) with the two R
 * of the unpermuted sample.  The entry does not know which side is X: to move X pass the inverse
 * permutation, Y as the held side and the row sums swapped (the same two mathematical sums).
 *
 * The held side is evaluated once per tw_hsic_perm_cols() columns (a chunk), the moved side per
 * column on gathered rows.  A workgroup owns a chunk and a run of consecutive tile pairs of the
 * triangle of tw_hsic_tile()-row tiles and leaves one double per column in d_work
 * (tw_hsic_perm_work_bytes bytes, nothing to zero); `wgs` > 0 bounds the workgroups per chunk
 * (ceil(pairs / ceil(pairs / wgs)) are used), wgs = 0 chooses (at most 512).  No atomics: a
 * column's partials and its Rab are added in a fixed order.  Results are run-to-run
 * deterministic, and a column's two doubles depend only on the data, on that column's index row
 * and on wgs — not on its position p, on n_cols or on the other columns.
 *
 * Every gathered index is clamped into [0, n) (as unsigned) before it addresses a row, so the
 * device reads inside the arrays whatever d_idx holds; the sums are unspecified for rows of d_idx
 * that are not permutations of 0 .. n - 1.  Masked pairs are selected to 0.0.  A NaN coordinate
 * on either side makes S_p NaN in every column (every permutation meets every row).  Under the
 * Gaussian kernel D = +inf gives g = exp(-inf) = 0 exactly (c < 0).  Under the distance kernel an
 * overflowing D = +inf gives g = sqrt(+inf) = +inf: the term H M is +inf, or NaN where the other
 * side's value is exactly 0 (equal rows), and S_p is +inf or NaN accordingly.
 *
 * TW_ERR_ARG before any device work: a null pointer, d_h or d_m outside [1, 64], n < 4 or
 * >= 2^31, n_cols < 1, an unknown kernel id, a non-finite or positive c_held or c_moved for the
 * Gaussian kernel, wgs < 0, a grid past 2^31 workgroups.  tw_hsic_perm_work_bytes is 0 for the
 * sizes tw_hsic_perm_sums refuses. */
int32_t tw_hsic_perm_cols(void);
int64_t tw_hsic_perm_work_bytes(int64_t n, int32_t n_cols, int32_t wgs);
int tw_hsic_perm_sums(const double* d_held, int32_t d_h, const double* d_moved, int32_t d_m,
                      int64_t n, const int32_t* d_idx, int32_t n_cols, const double* d_rows_held,
                      const double* d_rows_moved, int32_t kern, double c_held, double c_moved,
                      int32_t wgs, void* d_work, double* d_out, void* stream);

/* ---- Exact order statistics of pairwise squared distances (csrc/distselect.hip;
 * tuplewise.bandwidth; an extension): the pieces of a radix select over the bit
 * patterns of D, the squared distance of the triplet section (csrc/tripdist.h, the same device
 * functions, so a D has the bits every other entry gives it).  The pair sets:
 *   TW_DIST_WITHIN  the pairs i < j of d_x, (n, d) float64 row-major; d_z and m are ignored
 *   TW_DIST_CROSS   all (x_i, z_k) of d_x (n, d) and d_z (m, d)
 * 1 <= d <= 64, 0 <= n, m < 2^31.  The key of a pair is the 64-bit pattern of D.  For finite rows D
 * is never NaN and never -0 (it may be +inf by overflow, the largest key), bit 63 is 0 and keys
 * order as D does; rows with a non-finite entry are the caller's to refuse.
 *
 * A prefix group g is (prefix[g], prefix_bits[g]), 0 <= prefix_bits <= 63: a key belongs to it iff
 * its bits 62 .. 63 - prefix_bits[g], read as a number, equal prefix[g] (prefix_bits = 0 and
 * prefix = 0: every key).  `prefix` and `prefix_bits` are HOST arrays of n_groups entries, 1 <=
 * n_groups <= tw_dist_select_max_groups() (8); they are read before the call returns.  A digit is
 * bits [digit_shift, digit_shift + digit_bits) of a key, 1 <= digit_bits <=
 * tw_dist_select_digit_bits() (11), digit_shift + digit_bits <= 63.
 *
 * tw_dist_hist: d_hist is n_groups rows of 2^tw_dist_select_digit_bits() uint64 bins
 * (tw_dist_hist_bytes(n_groups) bytes, 0 for a refused n_groups); the call zeroes it, then
 *   d_hist[g * 2^bits + digit(key)] += 1   for every pair of the set and every group g the key
 *                                          belongs to
 * Each pair is visited once (tile pairs of tw_mmd_tile() rows a side as in tw_mmd_sums; a diagonal
 * tile counts anchor > point only) and the tile, tail and diagonal masks predicate the update: a
 * masked pair touches no bin.  Counts are integers added by integer atomics (uint32 bins per
 * workgroup in LDS, which a workgroup's 32768 pairs cannot overflow, then uint64 adds), so the
 * histogram is exact and run-to-run identical.
 *
 * tw_dist_gather: the same walk; every key that belongs to at least one group is written once to
 * d_keys (capacity entries) in an unspecified order.  d_count[0] = the number of such keys,
 * whatever the capacity; d_count[1] = 1 iff it exceeds the capacity, and then the keys past it are
 * dropped, never written.  The call zeroes d_count (2 entries).
 *
 * tw_keys_hist: tw_dist_hist's histogram of the n_keys entries of a key buffer.
 *
 * None of the three needs scratch.  TW_ERR_ARG before any device work: a null pointer (d_z for
 * TW_DIST_WITHIN and d_keys at capacity 0 may be NULL), an unknown pair set, d outside [1, 64], a
 * size outside [0, 2^31), n_groups outside [1, 8], prefix bits outside [0, 63] or a prefix wider
 * than them, a digit outside the limits above, a negative capacity or n_keys, a grid past 2^31
 * workgroups. */
#define TW_DIST_WITHIN 0
#define TW_DIST_CROSS 1
int32_t tw_dist_select_digit_bits(void);
int32_t tw_dist_select_max_groups(void);
int64_t tw_dist_hist_bytes(int32_t n_groups);
int tw_dist_hist(const double* d_x, int64_t n, const double* d_z, int64_t m, int32_t d,
                 int32_t pairs, const uint64_t* prefix, const int32_t* prefix_bits,
                 int32_t n_groups, int32_t digit_shift, int32_t digit_bits, uint64_t* d_hist,
                 void* stream);
int tw_dist_gather(const double* d_x, int64_t n, const double* d_z, int64_t m, int32_t d,
                   int32_t pairs, const uint64_t* prefix, const int32_t* prefix_bits,
                   int32_t n_groups, uint64_t* d_keys, int64_t capacity, uint64_t* d_count,
                   void* stream);
int tw_keys_hist(const uint64_t* d_keys, int64_t n_keys, const uint64_t* prefix,
                 const int32_t* prefix_bits, int32_t n_groups, int32_t digit_shift,
                 int32_t digit_bits, uint64_t* d_hist, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TUPLEWISE_H */
