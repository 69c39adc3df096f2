/*
 * somhip.h -- C ABI of the MI355X-native batch-SOM engine (libsomhip.so).
 *
 * The reference (jcfaracco/xpysom-dask) has no FFI layer of its own: its hot
 * path is reached through `xp.*` array calls inside the Python class XPySom.
 * This header is the boundary a drop-in replaces those calls with.  Every entry
 * point below names the reference code it stands in for (file:line under
 * /root/reference/xpysom_dask/).  The Python host (xpysom_dask_amd/xpysom.py)
 * binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every call returns 0 on success, non-zero on failure; the message is
 *     available from som_last_error(handle) (or som_last_error(NULL) when
 *     som_create itself failed).  Nothing throws across the ABI.
 *   - The caller owns all host buffers; the library owns all device buffers.
 *   - One handle = one GPU = one host thread at a time (not locked).
 *   - Codebook layout: float32 [K][D] row-major, K = X*Y, unit k = i*Y + j
 *     (xpysom.py:240 unravel table; distances.py:185 reshape).
 *   - Data layout: float32 [N][D] row-major (xpysom.py:510).
 */
#ifndef SOMHIP_H
#define SOMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct som_handle som_handle;

/* activation distance: distances.py:162-170 registry (names kept) */
enum { SOM_DIST_EUCLIDEAN = 0,        /* 'euclidean'  -> euclidean_squared_distance_part, distances.py:11-23 */
       SOM_DIST_EUCLIDEAN_NO_OPT = 1, /* 'euclidean_no_opt' -> euclidean_squared_distance, distances.py:25-31 */
       SOM_DIST_COSINE = 2,           /* 'cosine'     -> cosine_distance, distances.py:45-59 */
       SOM_DIST_MANHATTAN = 3,        /* 'manhattan', 'manhattan_no_opt' -> distances.py:109-158 (incl. the `l1norm` CUDA kernel) */
       SOM_DIST_NORM_P = 4,           /* 'norm_p' -> norm_p_power_distance, distances.py:98-107 (even p: binomial form :77-96) */
       SOM_DIST_NORM_P_NO_OPT = 5 };  /* 'norm_p_no_opt' -> norm_p_power_distance_generic, distances.py:61-75 */

/* neighbourhood function on the rectangular topology: neighborhoods.py:14-33, :57-74, :99-130 */
enum { SOM_NEIGH_GAUSSIAN = 0, SOM_NEIGH_MEXICAN_HAT = 1, SOM_NEIGH_BUBBLE = 2, SOM_NEIGH_TRIANGLE = 3 };

/* map topology: xpysom.py:196-206.  HEXAGONAL selects the *_generic neighbourhoods
 * (neighborhoods.py:35-55, :76-97) on the shifted-row coordinates; bubble ignores the shift.
 * TOROIDAL (not in the reference) is the rectangular grid with periodic boundaries on both axes: every neighbourhood
 * sees the offset to the NEAREST image of the BMU, d - L round(d / L) per axis (one image, never a sum), and the
 * support mask (bubble, compact_support) is -sigma < offset < sigma.  All four neighbourhoods; mexican_hat with
 * compact_support is refused. */
enum { SOM_TOPO_RECTANGULAR = 0, SOM_TOPO_HEXAGONAL = 1, SOM_TOPO_TOROIDAL = 2 };

/* arithmetic of the distance GEMM (the -2 x.w^T term, distances.py:22):
 *   F32  : v_mfma_f32_32x32x2_f32, exact float32 fma chain -- the parity mode
 *   BF16 : v_mfma_f32_16x16x32_bf16 on bf16-rounded x and w, f32 accumulate -- the throughput mode
 *   F16  : the BF16 kernels instantiated on IEEE half (v_mfma_f32_16x16x32_f16): 11 significant
 *           bits per operand instead of 8 at the same MFMA rate (97 % of the bf16 throughput under the chip's power
 *           limit); rows and units must fit float16 -- som_set_data / som_set_weights refuse rows and units whose
 *           norm exceeds 65504; streamed chunks and query rows (som_stream_rows, som_bmu) are not checked: values
 *           beyond the range saturate at +-65504
 *   EXACT: the BMUs of F32, row for row and bit for bit (near-ties and exact ties included), at half-precision MFMA
 *           speed: one pass of the MFMA kernel on power-of-two-scaled IEEE-half operands screens every unit and records
 *           the minimum of every 64-unit group per row (a group = a compact patch of the map: 8 x 8 units where both
 *           sides are multiples of 8), and the float32 fma chain itself re-scores the groups the
 *           screen's rigorous (partly measured) error bound cannot rule out; rows it cannot vouch for (NaN / infinite
 *           values, a pass with more candidate pairs than re-scoring is worth) go to the F32 kernel.  Euclidean distance
 *           with input_len <= 128; euclidean and cosine with 128 < input_len <= 800 on maps of >= 4096 units; other
 *           configurations run the F32 kernels under this id (which are the exact mode by definition).  On maps of >= 4096
 *           units the screen SKIPS the (256-row tile, block of units) pairs a centroid-and-radius bound proves empty
 *           (csrc/exact_skip.hpp, exact_skip_wide.hpp; SOM_EXACT_SKIP=0 runs every block): around last epoch's BMU for
 *           resident rows from their second epoch on (input_len <= 128; euclidean beyond), around a pseudo last BMU found
 *           from the current codebook's own group centroids for every other large row set -- query rows (som_bmu,
 *           som_bmu_device, som_quantization_error*), streamed chunks, a row set's first epoch.  A forecast on sample tiles
 *           declines plans with nothing to skip; the plan's own decisions come from timed costs of the handle's launches.
 *           The ids do not change, the time does, by the data.  Everything but the BMU search (update, merge,
 *           quantization) is as in F32. */
enum { SOM_PREC_F32 = 0, SOM_PREC_BF16 = 1,
       SOM_PREC_RETIRED_2 = 2,  /* was BF16X3 (hi/lo-split operands, three MFMAs per product): som_create refuses it --
                                   EXACT returns float32's own BMUs at three to ten times its speed; the id stays reserved */
       SOM_PREC_F16 = 3,      /* the bf16 path on IEEE half operands: 11 significant bits instead of 8, |value| <= 65504 */
       SOM_PREC_RETIRED_4 = 4,  /* was F16X3: refused likewise */
       SOM_PREC_EXACT = 5 };  /* F32's BMUs through an IEEE-half MFMA screen + float32 re-score (bmu_exact.hpp) */

/* Missing values (som_config.missing; not in the reference).  SOM_MISSING_NAN: a NaN in a training, streamed or query row means
 * "this feature was not observed" -- any NaN bit pattern (the test is x != x); +-inf is still a value.  With m_nd = 1 where x_nd is
 * observed and 0 otherwise, and x~_nd = x_nd where observed and 0 otherwise:
 *     BMU      b_n = the first minimum over k of s_nk = sum_d m_nd (x_nd - w_kd)^2, evaluated as fmaf(-2, c1, c2) with the two
 *              float32 fma chains c1 = sum_d x~_nd w_kd and c2 = sum_d m_nd fl(w_kd w_kd) (csrc/bmu_masked_f32.hpp).  A row with
 *              nothing observed scores 0 everywhere, takes unit 0 and adds nothing below.
 *     update   num[k][d] = sum_n g(b_n, k) m_nd x~_nd,   den[k][d] = sum_n g(b_n, k) m_nd,   g = eta h(b_n -> k) as ever;
 *              W[k][d] = num[k][d] / den[k][d] where den[k][d] != 0, otherwise W[k][d] stays bit for bit.  A denominator per
 *              unit AND feature: the fused accumulator is [K][round_up(2 input_len + 1, 4)], a row = [num (input_len) |
 *              den (input_len) | g-weighted row count | padding] -- som_accum_device_ptr, som_epoch_accumulate_block and
 *              som_epoch_allreduce report and move that size.  Sample weights w_n multiply both m_nd x~_nd and m_nd.
 *     QE       mean over ALL rows of sqrt(sum_d m_nd (x_nd - w_{b_n,d})^2), differences formed directly; a row with nothing
 *              observed adds 0 and is counted.
 * The codebook never receives a NaN from the data.  On complete rows num is the unmasked num bit for bit under the same BMUs
 * and every column of den is the unmasked den up to float32 summation order.
 * Scope: distance SOM_DIST_EUCLIDEAN; precision F32 or EXACT (both run the float32 masked kernel -- no screen applies);
 * every neighbourhood and topology; resident, device, weighted and streamed rows.  som_create refuses other distances and
 * BF16 / F16.  On such a handle som_epoch_fetch, som_epoch_accumulate_faithful, som_set_verify(n > 0), som_bmu_top2*,
 * som_bmu_f64 and som_distance_matrix fail with a message; som_epoch_fetch_masked reads the accumulator.
 * SOM_MISSING_NONE (the default): NaNs are ordinary values, every launch and result is what it is without this field. */
enum { SOM_MISSING_NONE = 0, SOM_MISSING_NAN = 1 };

/* which BMU rule som_bmu applies */
enum { SOM_BMU_ACTIVATION = 0,   /* configured activation distance: XPySom._winner, xpysom.py:410-417 */
       SOM_BMU_QUANTIZATION = 1  /* full sqrt'd Euclidean + nan_to_num: _quantization, xpysom.py:640,670 */ };

/* timed kernels for som_profile_get */
enum { SOM_K_BMU = 0, SOM_K_SEGSUM = 1, SOM_K_KRON = 2, SOM_K_MERGE = 3, SOM_K_PREP = 4,
       SOM_K_SCREEN = 5,   /* precision EXACT: the MFMA screen kernel alone (a part of SOM_K_BMU's time) */
       SOM_K_FILL = 6,     /* som_impute*: the fill of the completed rows alone (csrc/impute.hpp; its search is SOM_K_BMU's) */
       SOM_K_COUNT = 7 };

typedef struct som_config {
    int32_t x, y, input_len;     /* map rows, cols, features: XPySom.__init__, xpysom.py:73 */
    int32_t distance;            /* SOM_DIST_*  */
    int32_t neighborhood;        /* SOM_NEIGH_* */
    int32_t compact_support;     /* neighborhoods.py:29-31; with SOM_NEIGH_MEXICAN_HAT: the reference's double mask on px, :69-71 / :91-93 */
    int32_t precision;           /* SOM_PREC_*  */
    int32_t device;              /* HIP device ordinal */
    double  std_coeff;           /* d = 2*std_coeff^2*sigma^2, neighborhoods.py:19 */
    void*   stream;              /* hipStream_t to launch on; NULL = the library creates its own */
    int32_t topology;            /* SOM_TOPO_* */
    int32_t norm_p;              /* exponent p of SOM_DIST_NORM_P* (activation_distance_kwargs={'p': ...}); 0 = default 2 */
    double  norm_p_real;         /* a non-integer exponent p > 0 (distances.py:61-75 takes any real p); 0 = norm_p holds it */
    int32_t missing;             /* SOM_MISSING_* */
} som_config;

const char* som_version(void);
int         som_device_count(void);                      /* replaces utils.find_max_cuda_threads' device probe, utils.py:4-13 */
const char* som_last_error(const som_handle* h);

int  som_create(const som_config* cfg, som_handle** out); /* XPySom.__init__ device-side state, xpysom.py:193-240 */
void som_destroy(som_handle* h);

/* host <-> device codebook: train() entry/exit copies, xpysom.py:485, :580-583 */
int som_set_weights(som_handle* h, const float* w_host);
int som_get_weights(som_handle* h, float* w_host);

/* resident training data: xp.asarray(data, float32), xpysom.py:510.  The rows
 * stay on the device for all epochs.  _device: rows already in HBM (borrowed,
 * must outlive the handle's use of them). */
int som_set_data(som_handle* h, const float* x_host, int64_t n_rows);
int som_set_data_device(som_handle* h, const void* x_dev, int64_t n_rows);
/* Per-row sample weights of the resident rows, w_n >= 0 (scikit-style sample_weight):
 *     num[k] = sum_n w_n h(bmu_n -> k) x_n,   den[k] = sum_n w_n h(bmu_n -> k),   W[k] = num[k] / den[k] where den[k] != 0.
 * The BMUs are those of the unweighted call; the weights enter at one place, level 0 of the segment sum (csrc/update.hpp), where
 * a row adds w_n x_n to its BMU's sum and w_n to its count.  Weights of 1.0 give the unweighted epoch bit for bit; an integer
 * weight m counts the row m times; a row of weight 0 is not read at all (NaN / infinite features in it harm nothing); two
 * weighted epochs from the same state are bitwise equal.  Applies to som_epoch_accumulate, som_epoch, the staged form and
 * som_epoch_accumulate_forced; som_epoch_accumulate_faithful refuses to run while weights are set.
 *   som_set_sample_weights          float32 [n_rows] in host memory, copied to a buffer the library owns.  n_rows must be the
 *                                   resident row count; every value finite and >= 0 (checked on the host: the error names the first
 *                                   offending index).  w_host == NULL or n_rows == 0 clears the weights.
 *   som_set_sample_weights_device   float32 [n_rows] already in HBM, BORROWED like the rows of som_set_data_device (it must outlive
 *                                   the handle's use of it; order the engine behind its producer with som_sync_producer).  The
 *                                   CONTENTS ARE THE CALLER'S RESPONSIBILITY: nothing checks them, a negative, NaN or infinite
 *                                   weight goes into the sums as it is.  NULL / 0 clears.
 * som_set_data and som_set_data_device clear any weights: they belong to the rows they were set for. */
int som_set_sample_weights(som_handle* h, const float* w_host, int64_t n_rows);
int som_set_sample_weights_device(som_handle* h, const void* w_dev, int64_t n_rows);
/* ... whose producer may still be running: wait for it first.  `stream` is the producer's stream as the
 * __cuda_array_interface__ protocol names it (1 = legacy default, 2 = per-thread default, otherwise a
 * hipStream_t); has_stream == 0 = unknown producer, wait for the whole device.  (The reference's CuPy arrays
 * share CuPy's current stream with the kernels that read them, xpysom.py:487-510; here the engine owns a stream.) */
int som_sync_producer(som_handle* h, uint64_t stream, int32_t has_stream);
/* device rows of the caller copied to host memory (quantization_error(data) after train(device_rows, verbose=True),
 * xpysom.py:589-592 on a CuPy array) */
int som_copy_to_host(som_handle* h, const void* x_dev, uint64_t bytes, void* dst_host);

/* One epoch over the resident rows = the body of the epoch loop, xpysom.py:515-577:
 *   som_epoch_accumulate: w_sq cache (:529-537), every _update (:560-569 -> :420-443:
 *       BMU, neighbourhood*eta, sum_g, g^T x) summed into the fused float32
 *       accumulator [K][D+1] (numerator | denominator), left on the device;
 *   (multi-GPU: the host all-reduces the accumulator here -- replaces the Dask
 *       gather/sum, xpysom.py:545-558)
 *   som_epoch_merge: _merge_updates, xpysom.py:446-455.
 *   som_epoch = accumulate + merge.
 * sigma, eta: this epoch's schedule values (decays.py).  neigh_f64 != 0 evaluates
 * the neighbourhood in float64 (what NumPy >= 2 does when the schedule returns
 * numpy.float64, i.e. 'exponential'); 0 mimics the float32 evaluation. */
int som_epoch_accumulate(som_handle* h, double sigma, double eta, int neigh_f64);
/* the same accumulator computed the way the reference states it, xpysom.py:434-441: g = h * eta per (sample, unit)
 * generated from the neighbourhood tables inside a K x N x D float32 MFMA GEMM (num = g^T x, den = sum_n g), 2*N*K*D
 * flop where som_epoch_accumulate's bucketed algebra needs 2*K*(X+Y)*(D+1).  For cross-checks and the record. */
int som_epoch_accumulate_faithful(som_handle* h, double sigma, double eta, int neigh_f64);
int som_epoch_merge(som_handle* h);
int som_epoch(som_handle* h, double sigma, double eta, int neigh_f64);

/* som_epoch_accumulate in stages, for a host that overlaps the all-reduce with the tail of the epoch (the fused
 * accumulator is K*(D+1) floats -- 823 MB at 512x512x784 -- and the reference's gather/sum of it, xpysom.py:555-558,
 * is the one exchange step of the path):
 *   som_epoch_accumulate_begin    BMUs, segment sums, neighbourhood tables, stage 1 of the separable transform
 *   som_epoch_block_count         number of map-row blocks of stage 2 (128 map rows each, in order)
 *   som_epoch_accumulate_block    stage 2 of block b; afterwards floats [offset, offset + n_floats) of the
 *                                 accumulator (som_accum_device_ptr) are final and may be all-reduced on another
 *                                 stream (ordered behind som_get_stream's) while the next block is computed.
 * All blocks, then som_epoch_merge, equal som_epoch_accumulate + som_epoch_merge bit for bit. */
int som_epoch_accumulate_begin(som_handle* h, double sigma, double eta, int neigh_f64);
int som_epoch_block_count(som_handle* h, int32_t* n_blocks);
int som_epoch_accumulate_block(som_handle* h, int32_t block, int64_t* offset, int64_t* n_floats);

/* The same epoch for rows that do NOT stay resident (more rows than HBM holds, or a producer that
 * hands them over chunk by chunk -- what the reference gets from Dask blocks, xpysom.py:545-556):
 *   som_stream_begin                  w_sq cache, zero the segment sums
 *   som_stream_rows(x_host, n) ...    one _update per chunk: BMU + segment sums, added up on the device
 *   som_stream_end(sigma, eta, f64)   separable transform -> fused accumulator (then all-reduce / merge as above)
 * The sums of all chunks equal som_epoch_accumulate over their concatenation (float32 add order aside). */
/* A chunk in PINNED host memory (som_pinned_alloc, hipHostMalloc, hipHostRegister) is copied on a second
 * stream into one of two device slots, so its transfer overlaps the previous chunk's kernels; the buffer of
 * call i may be reused once call i+1 has returned (or after som_stream_end + som_sync).  A pageable chunk is
 * copied synchronously and is free on return. */
int som_pinned_alloc(uint64_t bytes, void** out);
int som_pinned_free(void* p);
int som_stream_begin(som_handle* h);
int som_stream_rows(som_handle* h, const float* x_host, int64_t n_rows);
/* a chunk with its sample weights (w_host: float32 [n_rows], finite and >= 0, checked on the host; see som_set_sample_weights).
 * They travel the way the rows do: with a pinned x_host on the copy stream into the device slot, else synchronously.  Weighted
 * and unweighted chunks may follow each other; an unweighted chunk's rows count 1 each. */
int som_stream_rows_weighted(som_handle* h, const float* x_host, const float* w_host, int64_t n_rows);
int som_stream_end(som_handle* h, double sigma, double eta, int neigh_f64);

/* The exchange step inside the library: one process per GPU, RCCL (bound at run time with dlopen -- the copy a host
 * such as torch already loaded, else librccl.so.1) all-reduces the fused accumulator over xGMI.  Replaces the Dask
 * gather -> sum -> broadcast of xpysom.py:545-558 for a caller that has nothing but this header:
 *   rank 0: som_comm_unique_id(id)  -> the host hands the 128 bytes to every rank (MPI, a file, a socket, ...)
 *   every rank: som_comm_init(h, world, rank, id)   collective; afterwards som_epoch() all-reduces between
 *                                   accumulate and merge (block by block under the transform when the map has
 *                                   more than one 128-row block), and som_epoch_allreduce() does the same for a host
 *                                   that drives accumulate / merge itself
 *   som_comm_destroy(h)             before som_destroy, on every rank
 * som_comm_load(path) picks the RCCL library explicitly (optional; NULL = the search described above). */
#define SOM_COMM_ID_BYTES 128
int som_comm_load(const char* librccl_path);
int som_comm_unique_id(void* id_out);
int som_comm_init(som_handle* h, int32_t world, int32_t rank, const void* id_bytes);
int som_epoch_allreduce(som_handle* h);
int som_comm_destroy(som_handle* h);

/* device address and length (floats) of the fused accumulator, for an in-place
 * all-reduce by the host (RCCL via torch.distributed). */
int som_accum_device_ptr(som_handle* h, void** dev_ptr, int64_t* n_floats);
/* the HIP stream every launch of this handle goes to (som_config.stream, or the handle's own): lets the caller
 * order foreign work -- e.g. the RCCL all-reduce of the accumulator -- on it instead of synchronising the host */
int som_get_stream(som_handle* h, void** stream_out);
/* teacher-forced parity: copy the last accumulate's results to the host.
 * Any pointer may be NULL.  num [K][D], den [K], bmu [n_rows] (raveled ids). */
int som_epoch_fetch(som_handle* h, float* num, float* den, int32_t* bmu);
/* ... of a handle created with SOM_MISSING_NAN (som_epoch_fetch refuses those, and this call the others):
 * num [K][input_len], den [K][input_len] -- a denominator per unit and feature --, bmu [n_rows].  Any pointer may be NULL. */
int som_epoch_fetch_masked(som_handle* h, float* num, float* den, int32_t* bmu);
/* teacher-forcing the other way: run the accumulate with these BMU ids instead
 * of computing them (isolates the update path in tests). */
int som_epoch_accumulate_forced(som_handle* h, const int32_t* bmu_host, double sigma, double eta, int neigh_f64);

/* BMU ids for arbitrary rows: XPySom.winner, xpysom.py:370-408 (mode ACTIVATION)
 * and XPySom._quantization, xpysom.py:632-645 (mode QUANTIZATION). */
int som_bmu(som_handle* h, const float* x_host, int64_t n_rows, int32_t mode, int32_t* ids_out);
/* ... for rows that already live in HBM (float32 [n_rows][input_len], borrowed for the call; order the engine behind their
 * producer with som_sync_producer first): no host round trip -- what the reference's winner() is on a CuPy array
 * (xpysom.py:379-396).  ids_out: host memory.  In EXACT precision large row sets run under a plan (the scout of
 * csrc/exact_skip.hpp gives every row a pseudo last BMU from the current codebook's own group centroids): the same ids,
 * a fraction of the distance GEMM. */
int som_bmu_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t mode, int32_t* ids_out);
/* best and second-best unit per row under the full Euclidean distance (sqrt + nan_to_num):
 * what XPySom.topographic_error takes from argsort(distances)[:, :2], xpysom.py:727-734.  Equal distances go to the lower
 * id first.  A map of one unit has no second-best: both ids are then 0. */
/* float64 query rows (XPySom.winner does not coerce its input, xpysom.py:379-396: float64 x against float32 weights is
 * computed in float64 by NumPy): the BMUs of fl64(-2 x.w + |w|^2_f32), euclidean activation distance only.  An analysis
 * call on the vector ALU; rows are staged through device memory as doubles. */
int som_bmu_f64(som_handle* h, const double* x_host, int64_t n_rows, int32_t* ids_out);
int som_bmu_top2(som_handle* h, const float* x_host, int64_t n_rows, int32_t* ids1_out, int32_t* ids2_out);
/* ... for rows that already live in HBM (see som_bmu_device: borrowed for the call, the same argument checks, at most
 * 2^31-1 rows; ids1_out / ids2_out: host memory).  In EXACT precision with the 'euclidean' activation distance up to 128
 * features both calls run the half-precision screen with its window on the SECOND-smallest group minimum, one select and the
 * float32 re-score twice (csrc/bmu_exact.hpp, "TOP-2"); every row whose pair a tie under the sqrt could reorder, or that the
 * screen cannot vouch for, is answered by the float32 top-2 kernel, so the ids are F32 precision's bit for bit.  Every other
 * configuration -- cosine, more than 128 features, F32 / BF16 / F16 -- runs the float32 kernel for every row, as does a handle
 * created with SOM_EXACT_TOP2=0 in the environment. */
int som_bmu_top2_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t* ids1_out, int32_t* ids2_out);
/* the (n_rows, K) distance matrix itself, row-major, for the analysis calls that return it:
 * mode ACTIVATION = XPySom.activate (xpysom.py:323-354, configured GEMM-form distance),
 * mode QUANTIZATION = XPySom.distance_from_weights (xpysom.py:647-671).  Never used while training. */
int som_distance_matrix(som_handle* h, const float* x_host, int64_t n_rows, int32_t mode, float* dist_out);
/* mean_n |x_n - W[bmu_n]|: XPySom.quantization_error, xpysom.py:673-707.  The distance to the chosen unit is
 * always evaluated exactly (float32 differences, float64 sum).  The BMU search is the reference's sqrt'd
 * Euclidean argmin in F32 precision; in BF16 / F16 precision with the 'euclidean' activation distance it
 * runs through the configured MFMA path (same argmin up to the operand rounding), as does som_bmu's
 * QUANTIZATION mode. */
int som_quantization_error(som_handle* h, const float* x_host, int64_t n_rows, double* qe_out);
/* ... of rows that already live in HBM (see som_bmu_device).  In EXACT precision with the 'euclidean' activation distance
 * the BMU search of both calls starts with the screen + float32 re-score (the float32 argmin of |w|^2 - 2 x.w).  That is
 * not always float32's argmin of the sqrt'd distance: where |x|^2 is large against the distances the radicand rounds or
 * clamps to 0, units at DIFFERENT distances tie under the sqrt, and the lowest id wins.  Every row whose pick such a tie
 * could overturn is searched again by the float32 SQRT kernel, so the ids -- and the value -- are F32 precision's. */
int som_quantization_error_device(som_handle* h, const void* x_dev, int64_t n_rows, double* qe_out);
/* Map diagnostics: the per-row terms of that mean, and how they spread over the map (not in the reference).
 *   b_n   the unit som_bmu(QUANTIZATION) names for row n on this handle: the Euclidean first minimum (SOM_MISSING_NAN: the masked
 *         search's), found as som_quantization_error finds it -- in EXACT precision through the screen and its tie window
 *   d_n   float32: |x_n - W[b_n]| exactly as som_quantization_error forms it before it widens and adds (SOM_MISSING_NAN: over the
 *         row's observed features; a row with nothing observed has b_n = 0, d_n = 0).  The novelty / outlier score of the row.
 * som_bmu_distances*: ids_out [n_rows] = b_n, dist_out [n_rows] = d_n, host memory; one of the two may be NULL, not both.
 * n_rows == 0 writes nothing.
 * som_unit_stats*: for every unit k (K = x * y entries per array, host memory; none may be NULL)
 *   count[k] = #{n : b_n = k}   sum[k] = sum d_n   sumsq[k] = sum d_n^2 (both in double; each square is exact)   max[k] = max d_n
 * and all four are 0 for a unit without rows (n_rows == 0: K zeros each).  The mean distance per unit -- the quantization-error
 * map -- is sum / count, the variance sumsq / count - mean^2; the raw quantities add across shards.  The sums run over a unit's
 * rows in ascending row index in a fixed reduction tree, without floating-point atomics: two calls on the same rows, and the host
 * and the device entry point on the same rows, return the same bits.  On a handle without SOM_MISSING_NAN a row holding a NaN
 * has d_n = NaN, and its unit's sum and sumsq are NaN; the counts stay exact and max ignores the NaN.
 * The *_device forms read rows that already live in HBM (see som_bmu_device: borrowed for the call, at most 2^31-1 rows). */
int som_bmu_distances(som_handle* h, const float* x_host, int64_t n_rows, int32_t* ids_out, float* dist_out);
int som_bmu_distances_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t* ids_out, float* dist_out);
int som_unit_stats(som_handle* h, const float* x_host, int64_t n_rows, int64_t* count, double* sum, double* sumsq, float* max);
int som_unit_stats_device(som_handle* h, const void* x_dev, int64_t n_rows, int64_t* count, double* sum, double* sumsq, float* max);
/* Missing values, the completed rows (not in the reference; csrc/impute.hpp): each NaN of a row replaced by what the row's unit
 * holds for that feature.  Only on a handle created with SOM_MISSING_NAN.
 *   a_n   the unit som_bmu(ACTIVATION) names for row n on this handle and codebook: the masked search of csrc/bmu_masked_f32.hpp,
 *         unchanged (a row with nothing observed takes unit 0)
 *   out[n][d] = x[n][d]      where x[n][d] is observed (x == x), BIT FOR BIT: -0.0, +-Inf and denormals as they are
 *   out[n][d] = W[a_n][d]    where x[n][d] is a NaN of any bit pattern: the float32 codebook value, bit for bit
 * A row with nothing observed becomes W[0]; a complete row is returned as it is and touches no codebook memory.  No arithmetic is
 * done on a value, so there is no tolerance: two calls, and the host and the device entry point on the same rows, return the
 * same bits.  A codebook that itself holds a NaN (som_set_weights: the caller's doing) hands that NaN on.
 * ids_out [n_rows] = a_n, host memory, or NULL.  n_rows == 0 writes nothing and returns 0.
 * som_impute: x_host and out_host are float32 [n_rows][input_len] host arrays; the rows are staged as som_bmu stages them and
 *   the result is copied back.  out_host == x_host is allowed.
 * som_impute_device: x_dev as in som_bmu_device (borrowed for the call, the same argument checks, at most 2^31-1 rows; order the
 *   engine behind the producers of BOTH arrays with som_sync_producer first).  out_dev: float32 [n_rows][input_len] in HBM, the
 *   caller's; every element is stored.  out_dev == x_dev fills in place: only the NaNs are stored, every element is read before
 *   it is written and by no other lane.  Neither pointer needs any alignment beyond a float's (aligned arrays with input_len % 4
 *   == 0 move 16 bytes a lane).  The call returns only after the fill has completed on the handle's stream: any stream of the
 *   caller may then read out_dev.
 * Refused, with a message that names the call: a handle without SOM_MISSING_NAN; a NULL row or out pointer with n_rows > 0;
 * n_rows < 0; ranges of x and out that overlap without being the same array.
 * A query: resident rows, their ids, the weights, the monitor's state and the exact mode's plans stay as they were. */
int som_impute(som_handle* h, const float* x_host, int64_t n_rows, float* out_host, int32_t* ids_out);
int som_impute_device(som_handle* h, const void* x_dev, int64_t n_rows, void* out_dev, int32_t* ids_out);
/* Label and value maps (not in the reference): what the rows a unit wins carry -- class labels, or columns of numbers the map was
 * not trained on.  a_n = the unit som_bmu(ACTIVATION) names for row n on this handle: the configured distance and precision
 * (SOM_MISSING_NAN: the masked search), the ids XPySom.predict / labels_map use -- not b_n above.  Outputs are host arrays
 * [K][C] with K = x * y, k = i * y + j; none may be NULL; n_rows == 0 writes zeros.
 * som_unit_label_counts*: labels [n_rows] int32 class codes, C = n_classes:
 *   counts[k][c] = #{n : a_n = k and labels[n] = c}      a label outside [0, C) (-1 by convention) is "unlabelled": counted nowhere
 * som_unit_value_sums*: values [n_rows][C] float32, row-major, C = n_cols; a NaN is "not observed" for that column only (whatever
 * the handle's missing mode), +-Inf is a value:
 *   count[k][c] = #{n : a_n = k, values[n][c] not NaN}   sum[k][c], sumsq[k][c] = the sums of those values and of their squares, in
 *   double (a float32 and its square are exact in double).  The mean of column c in unit k is sum / count; the raw quantities add
 *   across shards and ranks (each call reports the rows it was given).
 * Integer counts; the sums without atomics, over a unit's rows in an order that is a function of the unit's row count and C alone
 * (csrc/project.hpp): two calls on the same rows, and the host and the device entry point on the same rows, return the same bits.
 * Refused: a NULL argument with n_rows > 0, n_rows < 0 or > 2^31-1, C < 1 or > 4096, K * C > 2^26.
 * The *_device forms read rows, labels and values that already live in HBM (see som_bmu_device: borrowed for the call). */
int som_unit_label_counts(som_handle* h, const float* x_host, const int32_t* labels_host, int64_t n_rows, int32_t n_classes, int64_t* counts);
int som_unit_label_counts_device(som_handle* h, const void* x_dev, const void* labels_dev, int64_t n_rows, int32_t n_classes, int64_t* counts);
int som_unit_value_sums(som_handle* h, const float* x_host, const float* v_host, int64_t n_rows, int32_t n_cols, int64_t* count, double* sum, double* sumsq);
int som_unit_value_sums_device(som_handle* h, const void* x_dev, const void* v_dev, int64_t n_rows, int32_t n_cols, int64_t* count, double* sum, double* sumsq);
/* Data density per unit (not in the reference; csrc/density.hpp): Ultsch's P-matrix -- for every unit, how many rows lie within a
 * radius of its weight vector.  The one map diagnostic that does not follow from BMU ids: a full n_rows x K x input_len scan, run
 * on the float32 MFMA with a counting epilogue, the (n_rows, K) distances never written.  For radii r_1 .. r_R (1 <= R <= 8, host
 * floats) and a pivot c (input_len host floats; NULL: no centring):
 *   counts[j][k] = #{ n : sq(n, k) <= r2_j }      host array [n_radii][K], K = x * y, k = i * y + j
 *   r2_j = float32(r_j * r_j), the product formed in double;   x' = fl32(x - c),  w' = fl32(w - c);
 *   sq(n, k) = fl32( fmaf(-2, x'_n . w'_k, |w'_k|^2) + |x'_n|^2 ), the dot product a k-ordered float32 fma chain, each norm a
 *   float32 sum of the rounded squares in one fixed order.  The comparison is inclusive.
 * Always Euclidean and always float32, whatever the handle's activation distance and precision are (as som_quantization_error's
 * distance is).  The GEMM form cancels on un-centred data; distances are translation invariant, so the caller passes a pivot near
 * the data -- XPySom.density_map passes the midrange of the codebook, float32((min_k w_kd + max_k w_kd) / 2), which keeps
 * small-integer data exact.  A row that holds a NaN or +-Inf is counted for no unit.
 * Integer counts, added with integer atomics only: the same rows give the same counts in every call and under every launch
 * geometry, and the host and the device entry point agree; counts of separate calls (chunks, shards, ranks) add.
 * n_rows == 0 writes zeros.  Refused, with a message that names the call: a NULL radii / counts / rows pointer, n_rows < 0 or
 * > 2^31-1, n_radii outside 1 .. 8, a radius that is negative, NaN or whose square is not finite in float32, and a handle created
 * with SOM_MISSING_NAN (a distance over a row's observed features has no common scale across rows).
 * A query: resident rows, their ids, the weights, the monitor's state and the exact mode's plans stay as they were.  Scratch is
 * the handle's (the centred codebook: K * input_len floats), grown on demand, freed by som_destroy.
 * The *_device form reads rows that already live in HBM (see som_bmu_device: borrowed for the call). */
int som_unit_density(som_handle* h, const float* x_host, int64_t n_rows, const float* pivot, const float* radii, int32_t n_radii, int64_t* counts);
int som_unit_density_device(som_handle* h, const void* x_dev, int64_t n_rows, const float* pivot, const float* radii, int32_t n_radii, int64_t* counts);
/* The k nearest units of every row (not in the reference; csrc/topk.hpp): the ranked list behind smoothed data histograms, soft
 * labelling over the map, projection between units and rank-based topology measures.  The float32 MFMA scan with a top-k epilogue:
 * the (n_rows, K) score matrix is never written.  ONE definition:
 *   s_nk = the float32 activation score the float32 kernels compare for the handle's distance -- euclidean: fmaf(-2, x.w, |w|^2);
 *   euclidean_no_opt: that + |x|^2; cosine: 1 - nan_to_num(x.w / sqrt(|x|^2 |w|^2)) -- with x.w the k-ordered float32 fma chain of
 *   v_mfma_f32_32x32x2_f32 starting from 0 and the norms in NumPy's pairwise order: bit for bit the entries of som_distance_matrix
 *   (XPySom.activate) in SOM_BMU_ACTIVATION mode.
 *   The list of row n: the k units with the smallest s_nk, ascending; equal scores (-0.0 == +0.0) go to the lower unit id first -- a
 *   stable sort by (score, id).  A score enters only if it is < +inf: NaN and +inf never do (-inf does).  A slot that cannot be
 *   filled holds id -1, score NaN, distance NaN.  (cosine: nan_to_num turns a NaN quotient into score 1, as in som_distance_matrix.)
 * Always float32 arithmetic, whatever the handle's precision: on 'f32' and 'exact' handles slot 0 is som_bmu's ACTIVATION id for every
 * row that has a score below +inf.
 *   ids_out[n][j], score_out[n][j], dist_out[n][j]: host arrays, row-major (n_rows, k); score_out and dist_out may be NULL.
 *   dist[n][j] = sqrt(sum_d (x_nd - W[id][d])^2), the differences formed directly, in som_bmu_distances' arithmetic (same lanes, fma
 *   chain, wave sum, sqrtf) -- always Euclidean, as som_quantization_error's distance is, and NOT what orders the list: with a
 *   Euclidean activation it ascends along a row only up to rounding.  Skipped when dist_out is NULL.
 * som_unit_rank_counts*: counts[j][u] (host array [k][K]) = the number of rows whose slot j holds unit u, counted on the device from the
 * id lists -- the (n_rows, k) lists never leave HBM.  Integer atomics only: the same rows give the same counts in every call and
 * under every launch geometry; the counts of separate calls (chunks, shards, ranks) add.  n_rows == 0 writes zeros.
 * 1 <= k <= SOM_TOPK_MAX.  Refused, with a message that names the call: a NULL ids_out / counts / rows pointer, n_rows < 0 or
 * > 2^31-1, k outside 1 .. SOM_TOPK_MAX, k > K = x * y, a handle created with SOM_MISSING_NAN (as som_bmu_top2), a distance other
 * than euclidean, euclidean_no_opt, cosine (as som_distance_matrix), input_len >= 2^24.
 * The codebook is scanned in parts where few rows would not fill the chip, the parts' lists merged by (score, id): the result is
 * identical for every part count.  Rows run in passes of 262 144, so the scratch is bounded (the handle's, grown on demand, freed
 * by som_destroy).  A query: resident rows, their ids, the weights, the monitor's state and the exact mode's plans stay as they were.
 * The *_device form reads rows that already live in HBM (see som_bmu_device: borrowed for the call). */
#define SOM_TOPK_MAX 8
int som_bmu_topk(som_handle* h, const float* x_host, int64_t n_rows, int32_t k, int32_t* ids_out, float* score_out, float* dist_out);
int som_bmu_topk_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t k, int32_t* ids_out, float* score_out, float* dist_out);
int som_unit_rank_counts(som_handle* h, const float* x_host, int64_t n_rows, int32_t k, int64_t* counts);
int som_unit_rank_counts_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t k, int64_t* counts);

/* Row moments, for the codebook initialisers (not in the reference; csrc/moments.hpp).  With d_n = x_n - pivot formed in float32
 * (pivot: input_len host floats, NULL = 0) and w_n the row's weight (NULL = 1):
 *   *wsum = sum_n w_n      s1[a] = sum_n w_n d_na      gram[a][b] = sum_n w_n d_na d_nb      (host arrays: s1 [input_len], gram
 *   [input_len][input_len], full and symmetric -- gram[a][b] and gram[b][a] are the same bits; gram == NULL: only the sums, the
 *   cheap memory-bound pass).  Any pivot is exact for the covariance: cov = (gram - s1 s1^T / wsum) / divisor.
 * wsum and s1 add exact double products in double.  gram: fl(w_n d_na) * d_nb on v_mfma_f32_32x32x2_f32, a float32 chain per chunk
 * of SOM_MOMENTS_CHUNK_ROWS rows (include/somhip_test.h), the chunks' results added in double.  A row of weight 0 is left out as in
 * training: its features reach no sum, whatever they hold.  Weights of 1.0 give the unweighted call bit for bit.  There is no NaN
 * handling: a NaN or Inf in a contributing row makes s1 non-finite, which the caller tests.
 * No floating-point atomics; every order of addition is a function of (n_rows, input_len) alone: the same rows give the same bits
 * twice, and the device entry returns the host entry's bits (the host entry stages rows and weights and runs the same kernels).
 * A query: the handle's resident rows, their weights and ids and the exact mode's plans stay as they were.  Scratch is the
 * handle's, grown on demand, freed by som_destroy.
 * Refused: input_len > SOM_MOMENTS_MAX_FEATURES (before any launch), n_rows < 0 or > 2^31-1, a NULL wsum / s1 / rows pointer, a
 * negative or non-finite HOST weight (device weights are unchecked, as in som_set_sample_weights_device).  n_rows == 0 writes zeros.
 * The *_device form reads float32 rows [n_rows][input_len] and weights [n_rows] that already live in HBM (borrowed for the call;
 * see som_bmu_device).
 * som_gather_rows_device: out_host[i][:] = row idx_host[i] of the device block x_dev [n_rows][input_len], i < k; an index outside
 * [0, n_rows) is refused. */
#define SOM_MOMENTS_MAX_FEATURES 2048
int som_row_moments(som_handle* h, const float* x_host, const float* w_host, int64_t n_rows, const float* pivot, double* wsum, double* s1, double* gram);
int som_row_moments_device(som_handle* h, const void* x_dev, const void* w_dev, int64_t n_rows, const float* pivot, double* wsum, double* s1, double* gram);
int som_gather_rows_device(som_handle* h, const void* x_dev, int64_t n_rows, const int64_t* idx_host, int64_t k, float* out_host);

/* Training monitor (not in the reference): what an epoch did, measured from what the epoch itself left on the device -- the rows,
 * this epoch's BMU ids, the codebook W_t the epoch ran with (unchanged until som_epoch_merge) and the final accumulator.  No
 * second BMU search, no copy of the rows.  The epoch runs with W_t and produces W_{t+1}:
 *   sum_wd, sum_w   sum_n w_n d_n and sum_n w_n in double, over the rows of weight w_n > 0 (w_n = 1 without sample weights; a row
 *                   of weight 0 is not read).  d_n = the float32 |x_n - W_t[b_n]| exactly as som_bmu_distances forms it (SOM_MISSING_NAN:
 *                   over the observed features; a row with nothing observed has d_n = 0 and is counted), b_n = the unit THIS
 *                   EPOCH'S search found under the configured distance and precision.  The epoch's quantization error is
 *                   sum_wd / sum_w.  It is not som_quantization_error bit for bit: that call searches under the sqrt'd Euclidean
 *                   distance (other tie windows), and for the cosine, Manhattan and norm_p distances b_n is another unit.
 *   rows            rows measured (weight > 0)
 *   changed         rows whose b_n differs from the id the previous measured epoch left for the same resident row set; -1 = unknown:
 *                   the first measured epoch after som_set_data*, and every streamed epoch
 *   shift_sumsq     sum_{k,d} (W_{t+1}[k][d] - W_t[k][d])^2, differences and squares in double
 *   shift_max       max_{k,d} |W_{t+1}[k][d] - W_t[k][d]| in float32
 *                   W_{t+1}[k][d] is the float32 the merge will write: num / den where den != 0, else W_t[k][d] (SOM_MISSING_NAN: the
 *                   denominator of the feature).  Formed from the FINAL accumulator -- after the all-reduce --, so every rank
 *                   holds the same two values without a collective; the four row sums are this rank's and add across ranks.
 * Sums without floating-point atomics, in fixed trees over grids that depend on the row count and the map alone: two monitored
 * runs return the same bits.  A monitored schedule trains the codebook of the unmonitored one bit for bit.
 *   som_monitor(h, 1)           switches the monitor on: allocates its buffers and keeps a copy of every measured epoch's ids
 *                               beside the resident rows (som_set_data* invalidates it); som_monitor(h, 0) frees them.  While it
 *                               is off no call launches or allocates anything for it.
 *   som_epoch_measure_rows      launch; the resident rows, after any som_epoch_accumulate* form and before the next search
 *   som_epoch_measure_shift     launch; the accumulator must be final (after the all-reduce / the last staged block), before
 *                               som_epoch_merge
 *   som_epoch_metrics           ONE blocking read-back of the struct
 * Every launch is eager on the handle's stream (a replayed epoch graph is followed by them).  Streamed epochs: som_stream_begin
 * zeroes the row sums, every som_stream_rows* adds its chunk's in chunk order (som_epoch_measure_rows is implicit), and
 * som_epoch_metrics after som_stream_end (+ som_epoch_measure_shift) returns the totals.  som_epoch, the fused call, is not
 * monitored.  Errors (som_last_error): a measure call on a handle without som_monitor(h, 1); som_epoch_measure_rows with no
 * search since the last merge; som_epoch_measure_shift while staged blocks are outstanding. */
typedef struct { double sum_wd, sum_w, shift_sumsq; int64_t rows, changed /* -1: unknown */; float shift_max; } som_epoch_metrics_t;
int som_monitor(som_handle* h, int32_t on);
int som_epoch_measure_rows(som_handle* h);
int som_epoch_measure_shift(som_handle* h);
int som_epoch_metrics(som_handle* h, som_epoch_metrics_t* out);

/* The canary.  n_rows > 0: after every BMU launch (epochs, streamed chunks, som_bmu) n_rows strided rows are scored
 * again by the float32 parity kernel and the launch's own picks must be the float32 picks (F32, EXACT) or within the
 * precision mode's operand-rounding bound of them; otherwise the call fails with a message naming a row.  Costs one
 * small float32 launch and one host synchronisation per BMU launch: for smoke tests and stress runs (also: the
 * environment variable SOM_VERIFY=n at som_create).  som_verify_stats: launches / rows checked so far.
 * (The test hooks that go with it -- som_debug_* -- are declared in include/somhip_test.h, not here.) */
int som_set_verify(som_handle* h, int32_t n_rows);
int som_verify_stats(som_handle* h, int64_t* launches, int64_t* rows_checked);

/* precision EXACT, introspection (host arithmetic only, no device needed): the order in which the mode's operand images
 * hold the units of an x * y map -- perm_out[position] = unit id, x * y entries; every 64 consecutive positions are one
 * group of the screen / re-score: where both sides are multiples of 8 an 8 x 8 patch of the map held as four 4 x 4 blocks
 * (positions 0..15: rows 0..3 x columns 0..3 of the patch, row by row; 16..31: columns 4..7; 32..63: rows 4..7 likewise --
 * the 16-unit blocks the exact mode's plan tests); elsewhere a run of whole 8-row bands, ascending inside. */
int som_patch_order(int32_t x, int32_t y, int32_t* perm_out);

/* precision EXACT bookkeeping: rows screened so far, rows that went to the float32 fallback kernel, screen passes */
int som_exact_stats(som_handle* h, int64_t* rows, int64_t* rows_fallback, int64_t* passes);
/* top-2 bookkeeping (any precision): rows the top-2 calls served so far, and how many of them the float32 top-2 kernel
 * answered -- all of them on a handle that never takes the screen's path */
int som_exact_top2_stats(som_handle* h, int64_t* rows, int64_t* rows_f32);
/* precision EXACT, block skipping (csrc/exact_skip.hpp: resident rows from their second epoch on, input_len <= 128): how
 * many (256-row tile, 16-unit block) blocks the screens ran, of how many a full scan has -- the EXECUTED share of the
 * distance GEMM (launches without skipping count every block) */
int som_exact_skip_stats(som_handle* h, int64_t* blocks_run, int64_t* blocks_total);
/* ... and the resident sorted pass behind it: epochs that ran under a plan, and how many of them (re-)sorted the rows by
 * their last BMU's patch first (the others reused the order of an earlier epoch) */
int som_exact_resident_stats(som_handle* h, int64_t* planned_epochs, int64_t* sorts);
/* ... and the scout (csrc/exact_skip.hpp: pseudo last BMUs from the current codebook's own group centroids, for rows that
 * have no last BMU -- query rows, streamed chunks, a row set's first epoch -- and for a schedule's first epochs): BMU
 * launches that ran it, and launches over transient row sets (queries, streamed chunks) that ran under a plan */
int som_exact_scout_stats(som_handle* h, int64_t* scouted_launches, int64_t* transient_planned);
/* ... and the refinement pass between the screen and the float32 re-score (csrc/bmu_exact.hpp: both operands' second
 * half-precision halves, a window some twenty times narrower than the screen's): candidate (row, group) pairs it was
 * given, and how many of them it left for the re-score */
int som_exact_refine_stats(som_handle* h, int64_t* pairs_in, int64_t* pairs_out);
/* candidate groups per row of the LAST screen pass (its first n rows): how many 64-unit groups the select kernel found for the
 * row.  Under a plan (a sorted pass) entry i belongs to SORTED POSITION i of the pass, not to row i, and the counts are taken
 * BEFORE the refinement pass compacts the lists (som_exact_refine_stats has the totals on both sides of it). */
int som_exact_last_counts(som_handle* h, int32_t* counts_out, int64_t n);

/* stream / timing plumbing */
int som_sync(som_handle* h);
int som_profile_enable(som_handle* h, int32_t on);          /* hipEvent pairs around each kernel family (1), or around the
                                                               BMU kernels only (2: two event records per epoch); 0 = off */
int som_profile_get(som_handle* h, int32_t kernel, double* total_ms, int64_t* launches);
int som_profile_reset(som_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* SOMHIP_H */
