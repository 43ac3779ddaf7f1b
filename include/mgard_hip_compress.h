/* mgard_hip_compress.h -- C ABI of the HIGH-LEVEL path: whole-array compress / decompress with
 * domain decomposition, the lossless stage and the self-describing container, on top of the
 * low-level entry points of mgard_hip.h. Same shared library (libmgard_hip.so).
 *
 * What each entry point replaces in the reference (MGARD-X):
 *   mgh_compress / mgh_decompress   mgard_x::compress / decompress
 *                                   (include/compress_x.hpp:31-100, 109-154;
 *                                    CompressionHighLevel.hpp:47-330, 478-640)
 *   mgh_config                      mgard_x::Config (Config/Config.h:10-42, defaults Config.cpp:14-43)
 *   mgh_metadata_* / mgh_infer_*    Metadata<..>::Serialize / Deserialize, infer_shape,
 *                                   infer_data_type (Metadata/Metadata.hpp:226-262)
 *   mgh_huffman_*                   ComposedLosslessCompressor::Compress/Serialize and
 *                                   Deserialize/Decompress (Lossless/Lossless.hpp:70-118)
 *
 * Output container (byte-compatible with the reference, see mgard_amd/csrc/format.hpp):
 *   "MGARD" | u64 LE header_size | u32 LE crc32 | proto3 Header | per subdomain:
 *   [u64 compressed_size][payload]   (GPUPipelines.hpp:189-193), payload = the Huffman record
 *   of Huffman.hpp:163-239 (optionally [u64 size][zstd frame] around it, Zstd.hpp:69-90), or the
 *   raw subdomain when compression would not shrink it (GPUPipelines.hpp:136-155).
 *
 * Conventions as in mgard_hip.h. `original_data`, `compressed_data`, `decompressed_data` may be
 * host or device pointers (detected like MemoryManager::IsDevicePointer); when the output is not
 * pre-allocated the library allocates it in the same memory space as the input
 * (CompressionHighLevel.hpp:149-162): host outputs with malloc (release with free), device
 * outputs with hipMalloc (release with hipFree / mgh_free_device).
 */
#ifndef MGARD_HIP_COMPRESS_H
#define MGARD_HIP_COMPRESS_H

#include <stddef.h>
#include <stdint.h>

#include "mgard_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGH_ERR_OUTPUT_TOO_LARGE (-7) /* cf. compress_status_type::OutputTooLargeFailure */
#define MGH_ERR_FORMAT (-8)           /* malformed / unsupported compressed stream */
#define MGH_ERR_TARGET_NOT_MET (-9)   /* mgh_compress_target: not even tol_min meets the error target */

typedef enum mgh_domain_decomposition { /* domain_decomposition_type, Utilities/Types.h:50 */
  MGH_DD_MAXDIM = 0,
  MGH_DD_BLOCK = 1,
  MGH_DD_VARIABLE = 2
} mgh_domain_decomposition;

typedef enum mgh_lossless { /* lossless_type, Utilities/Types.h:33-38 */
  MGH_LOSSLESS_HUFFMAN = 0,
  MGH_LOSSLESS_HUFFMAN_LZ4 = 1, /* not supported: MGH_ERR_INVALID_ARGUMENT */
  MGH_LOSSLESS_HUFFMAN_ZSTD = 2,
  MGH_LOSSLESS_CPU = 3 /* not supported */
} mgh_lossless;

/* The fields of mgard_x::Config this path reads; mgh_config_default() fills the reference's
 * defaults (Config.cpp:14-43). */
typedef struct mgh_config {
  int dev_id;
  int domain_decomposition;      /* mgh_domain_decomposition */
  int domain_decomposition_dim;  /* Variable */
  const uint64_t *domain_decomposition_sizes; /* Variable: extent of every subdomain */
  uint64_t num_domain_decomposition_sizes;
  uint64_t block_size;           /* Block */
  double estimate_outlier_ratio;
  uint64_t huff_dict_size;
  uint64_t huff_block_size;
  int lossless;                  /* mgh_lossless */
  int zstd_compress_level;
  int normalize_coordinates;
  uint64_t max_larget_level;
  uint64_t max_memory_footprint; /* bytes of device memory the call may plan with */
  int auto_pin_host_buffers; /* default 0 here (reference: 1), see mgh_config_default */
  int reorder;               /* 0 (default): quantized integers in the N-D layout; 1: level by level
                                (Config::reorder, LinearQuantization.hpp:46-146) -- recorded in the header */
  int mirror_reference_coord_cast; /* decompression of a NON-uniform grid: 1 = coordinates through (float)
                                first, as the reference does even for double data
                                (CompressionHighLevel.hpp:455-462); 0 (default) = at full precision */
} mgh_config;

void mgh_config_default(mgh_config *config);

/* mgard_x::compress. coords: NULL (uniform) or D host arrays of the data type. If
 * output_pre_allocated, *compressed_size carries the capacity in and the size out. */
int mgh_compress(int D, int dtype, const uint64_t *shape, double tol, double s,
                 int error_bound_type, const void *original_data, void **compressed_data,
                 size_t *compressed_size, const void *const *coords, const mgh_config *config,
                 int output_pre_allocated);

/* ---- Sizes before compressing, and compression to a byte budget (extensions) -----------------------
 * What mgh_compress(tol) WOULD write, for `ntol` (1..64) tolerances, from one decomposition and one
 * read of the coefficients per launch of up to eight tolerances: the Huffman code is built from a
 * histogram and the record's layout is a formula, so a container's size follows from the histogram of
 * its symbols and its outlier count -- up to the padding of every Huffman chunk to a 64-bit unit,
 * which the histogram does not know. Hence a bracket, bytes_min <= size <= bytes_max, at most 8 bytes
 * per chunk (huff_block_size symbols) wide. code_bits: the bits of the Huffman codes; outliers: the
 * record's count; raw: 1 the writer will store the array itself (the record would not be smaller), 0 it
 * will not, -1 the bracket straddles that threshold.
 * Contract: containers of ONE subdomain (a configuration that decomposes the domain is
 * MGH_ERR_INVALID_ARGUMENT) and lossless = MGH_LOSSLESS_HUFFMAN (a Zstd frame's size is no function
 * of the histogram: MGH_ERR_INVALID_ARGUMENT). Host or device input, coords and config as in
 * mgh_compress. A REL bound with s != inf inherits the order dependence of the norm's last bits
 * (mgh_norm_stream_*): the estimate uses the reduction mgh_compress uses. */
typedef struct mgh_size_estimate {
  double tol;
  uint64_t bytes_min, bytes_max, outliers, code_bits;
  int raw;
} mgh_size_estimate;
int mgh_estimate_sizes(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s,
                       int error_bound_type, const void *original_data, const void *const *coords,
                       const mgh_config *config, mgh_size_estimate *out /* [ntol] */);

/* The most accurate container of at most max_bytes: searches [tol_min, tol_max] on a logarithmic
 * grid (tol_min if it fits; else `rounds` in 1..8 rounds of three candidates, which narrow the
 * bracket to (tol_max / tol_min)^(1 / 4^rounds)), pricing candidates as mgh_estimate_sizes does -- a
 * candidate fits when its bytes_max does, so the result fits by construction --, then writes the
 * container of *tol_used from the coefficients the candidates were priced on (no second decomposition):
 * the container is the one mgh_compress(*tol_used) writes, up to the order of its outlier list.
 * estimate_used (may be NULL): the estimate of *tol_used. The search is double-precision arithmetic
 * on the tolerances alone and reproducible bit for bit. MGH_ERR_OUTPUT_TOO_LARGE when not even
 * tol_max fits: nothing is allocated and *compressed_data is left as it was. tol_min <= 0,
 * tol_min > tol_max, rounds outside 1..8: MGH_ERR_INVALID_ARGUMENT. With output_pre_allocated,
 * *compressed_size carries the capacity in as in mgh_compress (max_bytes is the budget either way). */
int mgh_compress_budget(int D, int dtype, const uint64_t *shape, size_t max_bytes, double tol_min, double tol_max,
                        int rounds, double s, int error_bound_type, const void *original_data,
                        void **compressed_data, size_t *compressed_size, const void *const *coords,
                        const mgh_config *config, int output_pre_allocated, double *tol_used,
                        mgh_size_estimate *estimate_used /* may be NULL */);

/* ---- Achieved errors before compressing, and compression to an error target (extensions) -----------
 * A tolerance is a guaranteed bound, not the error a caller gets (mgh_verify exists because the two
 * differ). mgh_achieved_errors: out[k] holds the statistics mgh_verify (halvings = 0) would report for
 * the container mgh_compress(tols[k]) would write, for `ntol` (1..64) tolerances, from ONE
 * decomposition and WITHOUT writing a container: per tolerance the coefficients are turned into the
 * coefficients the decoder will see (mgh_quantize_roundtrip: one streaming pass, no integers, no
 * outlier lists, no lossless stage), recomposed (mgh_recompose) and compared with the input by the
 * kernel of mgh_compare. For a device-resident input every field equals mgh_verify's bit for bit; for a
 * host-resident one the exact fields (n, nonfinite, max_abs_err, argmax, the reference's extremes) do
 * and the two sums may round differently, as mgh_compare documents for host arrays.
 * Contract: containers of ONE subdomain (a configuration that decomposes the domain is
 * MGH_ERR_INVALID_ARGUMENT). The achieved error does not depend on the lossless stage: Huffman and
 * Huffman_Zstd are both accepted, as is either reorder. Host or device input, coords and config as in
 * mgh_compress. Device memory: the coefficient array and one more array of the input's size, both in
 * buffers the compression pipeline owns anyway.
 * Known limits. (1) A REL bound with finite s on float64 data inherits the order dependence of the
 * last bits of the norm (mgh_norm_stream_*): there the candidate and the written container may differ
 * in the last bits of their statistics. (2) Where mgh_compress stores the array itself because the
 * record would not be smaller (a RAW record: tiny arrays, or tolerances near the resolution of the
 * type) the container is exact, and the candidate's statistics -- the quantizer's -- are an upper bound
 * of its error rather than equal to it. */
typedef enum mgh_target_metric { MGH_TARGET_MAX_ABS = 0, MGH_TARGET_RMSE = 1, MGH_TARGET_PSNR = 2 } mgh_target_metric;
int mgh_achieved_errors(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s,
                        int error_bound_type, const void *original_data, const void *const *coords,
                        const mgh_config *config, mgh_error_stats *out /* [ntol] */);

/* The LARGEST tolerance in [tol_min, tol_max] whose achieved error meets `target` in `metric`
 * (max_abs_err <= target, rmse <= target, or psnr >= target; a result with non-finite positions meets
 * nothing), on a logarithmic grid: tol_max if it meets the target (1 candidate); else tol_min must
 * (2 candidates), and `rounds` (1..16) bisections in log, each one candidate evaluated as
 * mgh_achieved_errors evaluates it, narrow the bracket to (tol_max / tol_min)^(1 / 2^rounds). The
 * result meets the target BY MEASUREMENT, so an error curve that is not monotone costs compression at
 * worst, never the target. Then the container of *tol_used is written from the coefficients the
 * candidates share (no second decomposition): it is the one mgh_compress(*tol_used) writes, up to the
 * order of its outlier list. stats_used (may be NULL): the statistics of the chosen candidate;
 * candidates (may be NULL): how many were evaluated. The search is double-precision arithmetic on the
 * tolerances alone and reproducible bit for bit. MGH_ERR_TARGET_NOT_MET when not even tol_min meets the
 * target: nothing is allocated and *compressed_data is left as it was. metric outside 0..2, a NaN
 * target, tol_min <= 0, tol_min > tol_max, rounds outside 1..16: MGH_ERR_INVALID_ARGUMENT. The limits
 * of mgh_achieved_errors apply. */
int mgh_compress_target(int D, int dtype, const uint64_t *shape, int metric, double target, double tol_min,
                        double tol_max, int rounds, double s, int error_bound_type, const void *original_data,
                        void **compressed_data, size_t *compressed_size, const void *const *coords,
                        const mgh_config *config, int output_pre_allocated, double *tol_used,
                        mgh_error_stats *stats_used /* may be NULL */, int *candidates /* may be NULL */);

/* ---- One array at several tolerances: a ladder of containers (extension) ---------------------------
 * compressed_data[k] receives the container mgh_compress(tols[k]) writes for the same arguments (up to
 * the order of its outlier list), for `ntol` (1..64) tolerances in the order given -- fidelity tiers of
 * one array -- from ONE upload, ONE norm and ONE decomposition: the decomposition does not depend on the
 * tolerance, so every further tier costs a quantizer pass over the coefficients and a lossless stage.
 * Outputs live in the input's memory space and are allocated as mgh_compress allocates them (free them
 * the same way); with output_pre_allocated, compressed_size[k] carries the capacity of
 * compressed_data[k] in and the size out.
 * On a failure at tolerance k the status is the failing write's (MGH_ERR_OUTPUT_TOO_LARGE for a
 * pre-allocated buffer that is too small), containers 0 .. k-1 stay valid and stay the caller's, and
 * compressed_data[k ..] are NULL when the call allocates them.
 * Contract: containers of ONE subdomain (a configuration that decomposes the domain is
 * MGH_ERR_INVALID_ARGUMENT), either lossless type, either reorder. ntol outside 1..64 and a tolerance
 * that is not positive and finite: MGH_ERR_INVALID_ARGUMENT. Host buffers are not registered
 * (config->auto_pin_host_buffers is not honoured). Limit (1) of mgh_achieved_errors applies: a REL bound
 * with finite s on float64 data inherits the order dependence of the last bits of the norm, as two
 * mgh_compress calls do. Device memory: the coefficient array, and the symbols (2 bytes an element; 8,
 * and 8 more with reorder = 1, where the single-pass encoder does not run) in buffers of the pipeline. */
int mgh_compress_ladder(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s,
                        int error_bound_type, const void *original_data, void **compressed_data /* [ntol] */,
                        size_t *compressed_size /* [ntol] */, const void *const *coords, const mgh_config *config,
                        int output_pre_allocated);

/* ---- One array as precision LAYERS: containers that refine it, tolerance by tolerance (extension) -----
 * The tiers of a ladder are independent: each stores again what the coarser ones hold. Here
 * compressed_data[k] stores what layers 0 .. k-1 left: the decomposition is linear and does not depend on
 * the tolerance, so with r_0 the coefficients,
 *   q_k = quantize(r_k; tols[k])   (the level quantizers of tols[k], as mgh_quantize),
 *   r_{k+1} = r_k - dequantize(q_k; tols[k]),
 * and a reader adds dequantize(q_0) + ... + dequantize(q_k) before ONE recomposition (mgh_layers_*,
 * mgh_decompress_layers). After k layers every coefficient is off by at most half the level quantum of
 * tols[k] -- the error model of mgh_compress(tols[k]).
 * Every layer is an ordinary container of one subdomain with the header of tols[k]: compressed_data[0]
 * is the container mgh_compress(tols[0]) writes (up to the order of its outlier list), and a stock reader
 * decodes a later layer to a correction field. The containers carry NO layer index: their order is the
 * caller's to keep.
 * Arguments, outputs and the failure at layer k (containers 0 .. k-1 stay valid and the caller's) as in
 * mgh_compress_ladder. MGH_ERR_INVALID_ARGUMENT, before anything is allocated: ntol outside 1..64; a
 * tolerance that is not positive and finite; tolerances that are not STRICTLY DECREASING; a configuration
 * that decomposes the domain; config->reorder == 1; a huff_dict_size that is odd or outside 2..16384, or
 * one that, with huff_block_size, the single-pass encoder does not take; arrays of 2^32 elements and more.
 * A layer that would be stored RAW (the record is not smaller than the array: a tolerance below the
 * noise of the data) ends the call with MGH_ERR_INVALID_ARGUMENT, "compress_layers: layer k would be
 * stored raw". Either lossless type. Device memory: the coefficient array TWICE (a layer's residual must
 * not overwrite the coefficients it was made from until its record is written: an outlier overflow
 * quantizes them again) and the symbols (2 bytes an element), in buffers of the pipeline.
 * mgh_last_compress_stats: decompositions 1, records ntol, raw_records 0, quantize_passes ntol +
 * outlier_retries. */
int mgh_compress_layers(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s,
                        int error_bound_type, const void *original_data, void **compressed_data /* [ntol] */,
                        size_t *compressed_size /* [ntol] */, const void *const *coords, const mgh_config *config,
                        int output_pre_allocated);

/* ---- Precision layers in LEVEL ORDER: refinable by tolerance AND by resolution (extension) -------------
 * mgh_compress_layers with reorder = 1 records: the same chain q_k, r_{k+1}, the same arguments, outputs and
 * failure at layer k, but every record is level-linearised WHATEVER config->reorder says, so that a reader
 * takes level L of layer k from the head of that layer's record (mgh_level_layers_*). compressed_data[0]
 * is the container mgh_compress(tols[0]) writes with config->reorder = 1 (up to the order of its outlier
 * list); every layer is an ordinary container that mgh_decompress, mgh_decompress_level and
 * mgh_progressive_* open. The quantizing step is mgh_quantize_residual_linear (int64 integers: the
 * single-pass 16-bit encoder is not used, and its limits on huff_block_size do not apply).
 * MGH_ERR_INVALID_ARGUMENT as for mgh_compress_layers, minus config->reorder: ntol, the tolerances, a
 * configuration that decomposes the domain, huff_dict_size odd or outside 2..16384, arrays of 2^32 elements
 * and more, and "compress_level_layers: layer k would be stored raw". Device memory: the coefficient array
 * twice and the integers twice (8 bytes an element in a buffer of the pipeline and in one of the
 * hierarchy). mgh_last_compress_stats: decompositions 1, records ntol. */
int mgh_compress_level_layers(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s,
                              int error_bound_type, const void *original_data, void **compressed_data /* [ntol] */,
                              size_t *compressed_size /* [ntol] */, const void *const *coords, const mgh_config *config,
                              int output_pre_allocated);

/* What the last WRITING call of the calling thread did (mgh_compress, mgh_compress_budget,
 * mgh_compress_target, mgh_compress_ladder, mgh_compress_layers; thread-local; zeros before the first call; a failed call
 * leaves what it had counted). */
typedef struct mgh_compress_stats {
  uint64_t decompositions;     /* passes that turned data into coefficients (one per subdomain of
                                  mgh_compress; the estimators' own single one for the other three) */
  uint64_t quantize_passes;    /* passes that turned coefficients into integers or symbols for a record
                                  (candidates that were only priced or measured do not count) */
  uint64_t histogram_launches; /* launches of the lossless stage's own histogram kernel; a record whose
                                  bins the quantizer filled (mgh_quantize_symbols) counts 0 */
  uint64_t records;            /* records written, RAW ones included */
  uint64_t raw_records;        /* ... of which store the array itself */
  uint64_t outlier_retries;    /* quantizer passes repeated because the outlier lists overflowed */
} mgh_compress_stats;
int mgh_last_compress_stats(mgh_compress_stats *out);

/* mgard_x::decompress. Shape and type come from the header (query them first with
 * mgh_infer_shape / mgh_infer_data_type to pre-allocate). */
int mgh_decompress(const void *compressed_data, size_t compressed_size,
                   void **decompressed_data, const mgh_config *config,
                   int output_pre_allocated);

/* mgh_decompress into a buffer of the caller whose size and type the library CHECKS (against the
 * header it reads anyway, before anything is written): out_bytes must be exactly the bytes of the
 * array in the stream, out_dtype its type (MGH_ERR_INVALID_ARGUMENT otherwise). The reference's
 * pre-allocated form (compress_x.hpp:115-154) trusts the caller; this is the form for bindings that
 * hand over buffers of known size (extension). Host or device memory like mgh_decompress. */
int mgh_decompress_into(const void *compressed_data, size_t compressed_size, void *out, size_t out_bytes,
                        int out_dtype, const mgh_config *config);

/* One process, several devices (the reference's MGARD_ENABLE_MULTI_DEVICE switch is dead code,
 * include/mgard-x/RuntimeX/RuntimeX.h:53; its multi-GPU example runs one rank per GPU:
 * examples/mgard-x/CompressXgcData/TestXGCAbsoluteError.cpp:36-252). mgh_compress_multi takes a
 * HOST buffer (container in host memory) or a volume resident on ONE device (GPUPipelines.hpp:69-207
 * takes device pointers: the slabs of other devices travel there once, device to device --
 * hipMemcpyPeerAsync over xGMI --, the slabs of the source device are compressed where they are,
 * and the container comes back in device memory of the source device); a pre-allocated output
 * must be of the same kind as the input. mgh_decompress_multi: host buffers only. The domain
 * is cut into slabs of the slowest dimension, slab id runs on device dev_ids[id % num_dev] (one
 * host thread, stream set and cache per device; an id may be listed more than once); a REL
 * bound uses the norm of the WHOLE domain (slab norms combined on the host,
 * ErrorToleranceCalculator.hpp:69-89) and every slab the ABS bound of :134-155. The result is an
 * ordinary MGARD-X container with a MaxDim decomposition of dimension 0: mgh_decompress,
 * mgh_decompress_multi and stock MGARD-X read it; mgh_decompress_multi shares the subdomains of
 * any container decomposed that way out over the devices and hands everything else to
 * mgh_decompress on dev_ids[0]. config->dev_id is ignored. */
int mgh_compress_multi(int num_dev, const int *dev_ids, int D, int dtype, const uint64_t *shape,
                       double tol, double s, int error_bound_type, const void *original_data,
                       void **compressed_data, size_t *compressed_size, const void *const *coords,
                       const mgh_config *config, int output_pre_allocated);
int mgh_decompress_multi(int num_dev, const int *dev_ids, const void *compressed_data,
                         size_t compressed_size, void **decompressed_data,
                         const mgh_config *config, int output_pre_allocated);

/* One RANK per GPU over RCCL (the reference's own multi-GPU pattern: one MPI rank per device, each
 * compressing its block -- examples/mgard-x/CompressXgcData/TestXGCAbsoluteError.cpp:36-252). The
 * ranks' slabs of the SLOWEST dimension, in rank order, form one domain: every rank passes the
 * shape of ITS slab (dimensions 1.. equal on all ranks; all ranks hold the same number of planes,
 * the last one may hold fewer, at least 3) resident on config->dev_id. nccl_comm: the caller's
 * ncclComm_t of `nranks` ranks (passed as void *, so this header needs no rccl.h). Collectives, on
 * a stream of the library: ncclAllGather of the slab shapes and of the record sizes, ncclAllReduce
 * of ONE double for the norm a REL bound refers to (MAX for s = inf, SUM of squares otherwise:
 * ErrorToleranceCalculator.hpp:69-131; every slab then runs with the ABS bound of :134-155),
 * ncclSend / ncclRecv of the records to `root`, which writes the container mgh_compress would write
 * for a MaxDim decomposition of dimension 0 (GPUPipelines.hpp:189-193) -- in DEVICE memory of the
 * root (hipMalloc'ed unless pre-allocated; release with mgh_free_device). Other ranks get
 * *compressed_size = 0 and may pass compressed_data = NULL. coords: NULL, or D host arrays with the
 * rank's own slice of dimension 0 and the full arrays of the other dimensions.
 * mgh_decompress_dist is the mirror: the root holds the container (device memory), every rank gets
 * its slab back in d_local_out (device memory it allocated: mgh_infer_shape on the root tells the
 * global shape). Every rank must make the call; a rank that fails its argument checks returns before
 * the first collective, a failure later leaves the others inside RCCL until its time-out.
 * RCCL is resolved at first use: symbols already in the process (an application that links RCCL),
 * else librccl.so.1; mgh_dist_use_library(path) names the library the communicator was created with
 * when that is another one (e.g. the copy a Python framework bundles). With nranks == 1 the calls
 * run their first collective and then ARE mgh_compress / mgh_decompress (same bytes). */
int mgh_dist_use_library(const char *librccl_path);
int mgh_compress_dist(void *nccl_comm, int rank, int nranks, int root, int D, int dtype,
                      const uint64_t *local_shape, double tol, double s, int error_bound_type,
                      const void *d_local_data, void **compressed_data, size_t *compressed_size,
                      const void *const *coords, const mgh_config *config, int output_pre_allocated);
int mgh_decompress_dist(void *nccl_comm, int rank, int nranks, int root, const void *compressed_data,
                        size_t compressed_size, void *d_local_out, const mgh_config *config);

/* infer_shape / infer_data_type (Metadata.hpp:244-247). compressed_data: host or device. */
int mgh_infer_shape(const void *compressed_data, size_t compressed_size, int *D_out,
                    uint64_t *shape_out /* [MGH_MAX_DIM] */);
int mgh_infer_data_type(const void *compressed_data, size_t compressed_size, int *dtype_out);

/* ---- Reconstruction at a coarser level of the hierarchy (EXTENSIONS: the reference's public
 * decompress has no level argument; its refactoring layer has DataRefactor::Recompose(data,
 * start_level, stop_level, queue), DataRefactor.hpp:108-124) ------------------------------------
 * Levels are the hierarchy's: 0 = coarsest grid, l_target = the full array. `config` carries
 * max_larget_level as it does for mgh_decompress (the container does not record it; NULL =
 * defaults). Containers with ONE subdomain only: a domain-decomposed container answers
 * MGH_ERR_INVALID_ARGUMENT (every subdomain has its own hierarchy and l_target); for those, see
 * mgh_infer_coarsened_shape / mgh_infer_coarsened_nodes / mgh_decompress_coarsened below, which count
 * halvings of the grid instead of levels.
 *
 * mgh_infer_level_shape: shape of `level` and l_target of the container's hierarchy; level < 0:
 * only l_target (D_out / shape_out untouched). mgh_infer_level_nodes: index in the finest grid of
 * every node of `level` along `dim`, ascending (keep every second node and always the last one, per
 * coarsening); returns their number, or l_target for level < 0, or a negative status. With it a
 * caller picks the coordinates of the coarse grid of a non-uniform array. compressed_data: host or device
 * like mgh_infer_shape; with a host buffer neither call needs a device.
 *
 * mgh_decompress_level: like mgh_decompress (same memory-space rules: host or device stream, output
 * allocated in the stream's space unless pre-allocated), the output being the dense array of
 * mgh_infer_level_shape(level): mgh_dequantize_recompose_to_level of the decoded integers.
 * level == l_target returns the bytes of mgh_decompress. For a reorder = 0 record the lossless stage
 * decodes the whole record (the box of a level is spread over every chunk). A reorder = 1 record is
 * level-linearised: below l_target only its leading ceil(N_level / huff_block_size) Huffman chunks are
 * decoded (mgh_lossless_decompress_prefix) and the level is made from that head
 * (mgh_dequantize_recompose_linear_to_level) -- of a record in host memory only the head, the code
 * units of those chunks, the outlier lists and the synchronisation entries of those chunks are moved.
 * mgh_last_decompress_stats tells what the last call did. A record that was stored RAW (the data itself, because the lossless stage did not shrink
 * it) is returned as it is at l_target; below l_target it costs a full decomposition and
 * quantization with the header's bound first, so that the level is the one a Huffman record gives. */
int mgh_infer_level_shape(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                          int level, int *D_out, uint64_t *shape_out /* [MGH_MAX_DIM] */, int *l_target_out);
int mgh_infer_level_nodes(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                          int level, int dim, uint64_t *h_idx_out, uint64_t cap);
int mgh_decompress_level(const void *compressed_data, size_t compressed_size, int level,
                         void **decompressed_data, const mgh_config *config, int output_pre_allocated);

/* ---- Reduced resolution of ANY container, domain-decomposed ones included (EXTENSION) ---------------
 * `level` counts from the coarsest grid, and every subdomain has its own hierarchy and l_target, so
 * one level number means a different resolution in each subdomain. The number that means the same in
 * all of them is how often the grid has been halved: halvings = k >= 0. One halving turns an extent
 * n into n / 2 + 1 (keep every second node and always the last one -- the hierarchy's own rule).
 *
 * Subdomain i (shape and offset as mgh_decompress sees them; a Variable decomposition takes its sizes
 * from `config`) has l_target_i = the l_target of a hierarchy of its shape under
 * config->max_larget_level. K = min_i l_target_i is the largest k; k > K answers
 * MGH_ERR_INVALID_ARGUMENT (no subdomain is clamped: a block with fewer halvings than its neighbours
 * would break the tensor-product grid). Subdomain i is reconstructed at level l_target_i - k, bit for bit
 * what mgh_dequantize_recompose[_linear|_sym16]_to_level gives for it alone with the quantization
 * mgh_decompress uses for it, and the level arrays are stitched in decomposition-grid order into ONE
 * dense array: along dimension d the block at grid position j has the extent of n_{j,d} after k
 * halvings, its offset is the sum of the extents before it, the stitched extent the sum of all.
 * k = 0 returns the bytes of mgh_decompress; on a container with one subdomain k returns the bytes of
 * mgh_decompress_level(l_target - k).
 *
 * mgh_infer_coarsened_shape: shape of the stitched array and K; halvings < 0: only K (D_out /
 * shape_out untouched). mgh_infer_coarsened_nodes: index in the FULL array of every node of the
 * stitched grid along `dim`, ascending -- per block, its offset in the full array plus the nodes its
 * k halvings keep. The stitched grid is NOT uniform even for a uniform array (between two blocks the
 * step is one fine spacing), so coordinates of the result are always read through this list. Returns
 * the number of nodes, or K for halvings < 0, or a negative status. compressed_data: host or device;
 * with a host buffer neither call needs a device.
 *
 * mgh_decompress_coarsened: memory-space rules of mgh_decompress_level. A reorder = 1 container with
 * k > 0 decodes only the head of every record (mgh_last_decompress_stats accumulates over the
 * subdomains); a reorder = 0 container decodes every record whole; a RAW record costs, for k > 0, a
 * decomposition and quantization with the subdomain's bound first. A device output whose blocks are
 * whole slabs of dimension 0 is written in place. */
int mgh_infer_coarsened_shape(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                              int halvings, int *D_out, uint64_t *shape_out /* [MGH_MAX_DIM] */,
                              int *max_halvings_out);
int mgh_infer_coarsened_nodes(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                              int halvings, int dim, uint64_t *h_idx_out, uint64_t cap);
int mgh_decompress_coarsened(const void *compressed_data, size_t compressed_size, int halvings,
                             void **decompressed_data, const mgh_config *config, int output_pre_allocated);

/* EXTENSION: full-grid preview. The container after `halvings` coarsenings -- halvings, its range
 * check, one-subdomain containers and the records decoded exactly as in mgh_decompress_coarsened --
 * put back on the grid of the data: the output has the shape and type of mgh_infer_shape /
 * mgh_infer_data_type, in host or device memory like mgh_decompress. Every subdomain is reconstructed
 * at its level l_target_i - halvings, prolonged inside its own hierarchy to its full shape
 * (mgh_prolong) and placed where mgh_decompress places it; a device output whose subdomains are
 * whole slabs of dimension 0 is prolonged into in place. The contract is per subdomain: the result
 * there is, bit for bit, the recomposition of the subdomain's (dequantized) coefficient array with
 * everything outside the corner box of that level set to zero -- with the one exception mgh_prolong
 * has on 3-D subdomains of the fused route: a -0.0 of the level array at a node the next level keeps
 * stays -0.0 where the recomposition gives +0.0 (the sign of a zero, nothing else). Nothing is interpolated across
 * subdomain borders. halvings = 0 is mgh_decompress. Of a reorder = 1 container only the heads are
 * decoded (mgh_last_decompress_stats). */
int mgh_decompress_preview(const void *compressed_data, size_t compressed_size, int halvings,
                           void **decompressed_data, const mgh_config *config, int output_pre_allocated);

/* EXTENSION: windowed full-grid preview. The box W = [lo_d, lo_d + ext_d) per dimension (indices of
 * the array of mgh_infer_shape; lo and ext hold one uint64_t per dimension on the host; ext_d >= 1,
 * lo_d + ext_d <= shape_d, else MGH_ERR_INVALID_ARGUMENT) of what mgh_decompress_preview writes for the
 * same container and halvings, bit for bit: a dense array of shape ext, in host or device memory by
 * the rules of mgh_decompress_preview; the range check on halvings is the same. A subdomain whose box
 * does not meet W is not opened: nothing of it is decoded, none of its record bytes are moved (its
 * 8-byte size prefix is read, to find the next record), and it does not count in
 * mgh_last_decompress_stats, whose `subdomains` is the number of subdomains reconstructed. A
 * subdomain that meets W is reconstructed at l_target_i - halvings exactly as for the full preview,
 * and its part of W is written by mgh_prolong_window of its own hierarchy -- straight into a
 * device-resident output, else through a window-sized buffer. halvings = 0 is the crop of
 * mgh_decompress, with the same skipping. Nothing is interpolated across subdomain borders. */
int mgh_decompress_preview_window(const void *compressed_data, size_t compressed_size, int halvings, const uint64_t *lo,
                                  const uint64_t *ext, void **decompressed_data, const mgh_config *config,
                                  int output_pre_allocated);

/* EXTENSION: how far is a container from the data it was made from? mgh_error_stats (mgard_hip.h)
 * of `original` (the reference array, a) against what mgh_decompress -- halvings = 0 -- or
 * mgh_decompress_preview -- halvings > 0, with its range check -- would write (b), WITHOUT that
 * array ever existing. Every subdomain goes through the decoder's own path up to the dense
 * subdomain in its lane's buffer (halvings > 0: mgh_prolong last) and is then compared with the
 * same box of `original` by the kernel of mgh_compare: a device-resident original is read in place
 * through the box's offset and the array's strides, the box of a host-resident one is uploaded into
 * a second buffer of the lane. The partial results are folded in subdomain order (merge,
 * csrc/compare_plan.hpp); stats.argmax is the flat index in the FULL array. Device memory: the
 * lanes' buffers, plus one box per lane for a host original -- nothing of the size of the array.
 * original_bytes / original_dtype are checked against the header before any work, as
 * mgh_decompress_into checks its buffer (MGH_ERR_INVALID_ARGUMENT). Container and original may each
 * be in host or device memory.
 * The bound (halvings = 0 only): s = inf: bound_kind 0, achieved = stats.max_abs_err; s = 0:
 * bound_kind 1, achieved = sqrt(sum_sq_err / (n - nonfinite)) with config->normalize_coordinates,
 * else sqrt(sum_sq_err); bound = tol, or tol * the header's norm for a REL container; within =
 * achieved <= bound, and 0 whenever stats.nonfinite > 0. Any other s: the bound is in the s-norm,
 * which this call does not compute -- bound_kind = within = -1. halvings > 0: a preview carries no
 * bound, within = -1 (bound_kind and bound are still the header's); stats is the point. */
typedef struct mgh_verify_result {
  mgh_error_stats stats;
  int bound_kind;  /* 0: L-infinity (s = inf), 1: L2 (s = 0), -1: not evaluated */
  double bound;    /* absolute: tol, or tol * the header's norm for REL */
  double achieved; /* max_abs_err, or l2_error(config->normalize_coordinates) */
  int within;      /* 1 / 0 / -1 */
} mgh_verify_result;
int mgh_verify(const void *compressed_data, size_t compressed_size, const void *original, size_t original_bytes,
               int original_dtype, int halvings, const mgh_config *config, mgh_verify_result *out);

/* What the last mgh_decompress* call of the calling thread did in its lossless stage (thread-local;
 * zeros before the first call; a failed call leaves what it had counted). Raw records count in
 * subdomains and record_bytes only. */
typedef struct mgh_decompress_stats {
  uint64_t subdomains;
  uint64_t chunks_total;       /* Huffman chunks of the records */
  uint64_t chunks_decoded;     /* ... of which decoded */
  uint64_t symbols_decoded;    /* integers the decoders wrote */
  uint64_t record_bytes;       /* bytes of the records (Huffman_Zstd: of the frames) */
  uint64_t record_bytes_moved; /* bytes of the records copied to the device or within it; code
                                  units decoded in place count 0 */
} mgh_decompress_stats;
int mgh_last_decompress_stats(mgh_decompress_stats *out);

/* Stream contract of mgh_compress / mgh_decompress: the calls return when the result is
 * complete (they synchronise their own pipeline streams before returning). The pipeline streams
 * are created with default (blocking) flags like the reference's queues
 * (include/mgard-x/RuntimeX/DeviceAdapters/DeviceAdapterHip.h:514), i.e. they are ordered against
 * the NULL stream: a device-resident input that earlier work on the NULL stream is still
 * producing is complete before the first stage reads it. Work the caller has in flight on other
 * NON-BLOCKING streams is not waited for -- synchronise those before the call. */
/* pin_memory / check_memory_pinned / unpin_memory (compress_x.hpp:166-178): page-lock a host
 * buffer so that the pipeline's transfers out of / into it are asynchronous DMA. */
int mgh_pin_memory(void *ptr, size_t num_bytes);
int mgh_check_memory_pinned(const void *ptr); /* 1 = pinned, 0 = not */
int mgh_unpin_memory(void *ptr);
void mgh_free_device(void *p);
/* release_cache (compress_x.hpp:159): drops this thread's cached hierarchies and buffers, and the
 * idle scratch buffers of mgh_compare (those belong to the process, not to a thread). */
void mgh_release_cache(void);
/* Synchronous copy between any two of host / device memory (hipMemcpyDefault); lets a host
 * language without HIP bindings read the buffers the contexts own. */
int mgh_memcpy(void *dst, const void *src, size_t bytes);

/* ---- header (metadata) on its own: host only, no device needed -------------------------- */
typedef struct mgh_header_info {
  uint64_t version[3];
  int dtype;
  int D;
  uint64_t shape[MGH_MAX_DIM];
  int uniform;
  const double *coords[MGH_MAX_DIM]; /* !uniform: serialize reads them; parse points them into
                                        the caller's coords_storage */
  int error_bound_type; /* mgh_error_bound */
  double tol, s, norm;
  int domain_decomposed;
  int dd_method; /* mgh_domain_decomposition */
  uint64_t dd_dim, dd_size;
  uint64_t l_target;
  int reorder;
  int lossless; /* mgh_lossless */
  uint64_t huff_dict_size, huff_block_size;
} mgh_header_info;

/* Returns the number of bytes written (or needed when out == NULL), negative on error. */
int64_t mgh_metadata_serialize(const mgh_header_info *info, uint8_t *out, uint64_t capacity);
/* Parses preamble + header; *metadata_size_out = offset of the first subdomain record. */
int mgh_metadata_parse(const uint8_t *data, uint64_t size, mgh_header_info *info,
                       double *coords_storage, uint64_t coords_capacity,
                       uint64_t *metadata_size_out);

/* ---- lossless stage on its own (device pointers) ----------------------------------------- */
/* Host only: the canonical code built from a histogram, as it goes into the payload --
 * code[s] = (length << 56) | value (0: unused symbol), first[64] / entry[64] / keys[dict] with
 * the meaning Decode.hpp:52-106 gives them (reference GetCodebook.hpp:23-147 produces the
 * same three tables on the device). */
int mgh_huffman_codebook(const uint32_t *freq, uint64_t dict_size, uint64_t *code_out,
                         uint64_t *first_out /* [64] */, uint64_t *entry_out /* [64] */,
                         uint64_t *keys_out /* [dict_size] */);

/* Histogram of 16-bit symbols (mgh_decompose_quantize_sym16, mgh_quantize_symbols) as the lossless stage
 * counts them: d_freq[q] += the number of d_symbols[i] == q < dict_size (2..16384). THE CALLER ZEROES
 * d_freq. 1 .. 2^32 - 1 symbols. ASYNCHRONOUS on `stream`, on the current device. */
int mgh_histogram_sym16(const uint16_t *d_symbols, uint64_t n, uint64_t dict_size, uint32_t *d_freq, void *stream);

typedef struct mgh_lossless_ctx mgh_lossless_ctx;
int mgh_lossless_create(mgh_lossless_ctx **out, int dev_id);
void mgh_lossless_destroy(mgh_lossless_ctx *ctx);
/* Quantized symbols (int64 in [0, dict_size)) + outlier list -> serialized payload in a host
 * buffer owned by the context (valid until the next call); *size_out bytes. */
int mgh_lossless_compress(mgh_lossless_ctx *ctx, const int64_t *d_quantized, uint64_t n,
                          uint64_t dict_size, uint64_t chunk_size, int lossless, int zstd_level,
                          const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                          uint64_t outlier_count, const uint8_t **h_payload_out,
                          uint64_t *size_out, void *stream);
/* The same with the record written into DEVICE memory of the caller (d_record_out, any byte
 * alignment, `capacity` bytes): what the subdomain pipeline of mgh_compress does with every record
 * of a device-resident container -- the encoder stores its code units straight into the record
 * (GPUPipelines.hpp:189-193 lays the records out back to back, so a record starts wherever the
 * previous one ended). Huffman only (a Zstd frame is assembled on the host).
 * MGH_ERR_OUTPUT_TOO_LARGE when the record does not fit. */
int mgh_lossless_compress_device(mgh_lossless_ctx *ctx, const int64_t *d_quantized, uint64_t n,
                                 uint64_t dict_size, uint64_t chunk_size,
                                 const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                                 uint64_t outlier_count, void *d_record_out, uint64_t capacity,
                                 uint64_t *size_out, void *stream);
/* Inverse: payload (host, or device memory at any byte alignment) -> d_quantized [n], outlier
 * list in device buffers owned by the
 * context (*d_outlier_idx_out / *d_outlier_val_out, *outlier_count_out entries). */
int mgh_lossless_decompress(mgh_lossless_ctx *ctx, const uint8_t *h_payload, uint64_t size,
                            int lossless, int64_t *d_quantized, uint64_t n,
                            const uint64_t **d_outlier_idx_out, const int64_t **d_outlier_val_out,
                            uint64_t *outlier_count_out, void *stream);

/* The same for the first n_prefix integers only: chunks 0 ... ceil(n_prefix / chunk) - 1 are decoded,
 * d_quantized[0 ... min(n, chunks * chunk)) is written and nothing behind it (the buffer need not be
 * larger). The record's head is validated as a whole; the chunk-table entries are checked for the
 * chunks decoded. The outlier lists are delivered whole (they are not sorted). Of a record in HOST
 * memory only the head, the code units up to the end of the last needed chunk (plus the one unit the
 * decoders peek at), the outlier lists and the synchronisation entries of the needed chunks are
 * moved; a record on the decoding device is read in place; a Huffman_Zstd frame is inflated whole on
 * the host. n_prefix = n (or larger) is mgh_lossless_decompress; n_prefix = 0 is an error. */
int mgh_lossless_decompress_prefix(mgh_lossless_ctx *ctx, const uint8_t *payload, uint64_t size,
                                   int lossless, int64_t *d_quantized, uint64_t n, uint64_t n_prefix,
                                   const uint64_t **d_outlier_idx_out, const int64_t **d_outlier_val_out,
                                   uint64_t *outlier_count_out, void *stream);

/* The same for a RANGE of integers: chunks first / chunk ... (first + count - 1) / chunk are decoded;
 * d_quantized[0 ...) receives the integers from (first / chunk) * chunk to the end of the last decoded
 * chunk (or n), and nothing behind that. The head is validated as for the prefix call. Of a record in
 * host memory only the head, the code units and the synchronisation entries of the decoded chunks and
 * the (whole) outlier lists are moved. first = 0 is the prefix call; count = 0 or a range that leaves
 * [0, n) is an error. */
int mgh_lossless_decompress_range(mgh_lossless_ctx *ctx, const uint8_t *payload, uint64_t size, int lossless,
                                  int64_t *d_quantized, uint64_t n, uint64_t first, uint64_t count,
                                  const uint64_t **d_outlier_idx_out, const int64_t **d_outlier_val_out,
                                  uint64_t *outlier_count_out, void *stream);

/* ---- the same stage on 16-bit symbols (what mgh_compress moves through it when reorder = 0) ----
 * mgh_lossless_compress_sym16 / mgh_lossless_compress_device_sym16: mgh_lossless_compress[_device] with
 * the symbols as uint16_t (mgh_decompose_quantize_sym16, mgh_quantize_symbols); the record is the one
 * written from the same values as int64, byte for byte. The single-pass encoder only, which stages a
 * chunk's symbols and the code table in LDS: dict_size * 8 + chunk_size * 2 > 140 KiB is
 * MGH_ERR_INVALID_ARGUMENT. */
int mgh_lossless_compress_sym16(mgh_lossless_ctx *ctx, const uint16_t *d_symbols, uint64_t n,
                                uint64_t dict_size, uint64_t chunk_size, int lossless, int zstd_level,
                                const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                                uint64_t outlier_count, const uint8_t **h_payload_out,
                                uint64_t *size_out, void *stream);
int mgh_lossless_compress_device_sym16(mgh_lossless_ctx *ctx, const uint16_t *d_symbols, uint64_t n,
                                       uint64_t dict_size, uint64_t chunk_size,
                                       const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                                       uint64_t outlier_count, void *d_record_out, uint64_t capacity,
                                       uint64_t *size_out, void *stream);
/* Inverse into uint16_t symbols: first = 0, count = n decodes the whole record into d_symbols[0 .. n);
 * anything else has the chunk-range semantics of mgh_lossless_decompress_range (count = 0 or a range
 * that leaves [0, n) is an error). Nothing but 2-byte elements is ever written to d_symbols: a record
 * that the decoder with a 16-bit output does not take -- chunk_size < 1024, a code longer than 32 bits,
 * or MGH_HUFF_SERIAL_DECODE / MGH_HUFF_PAR_DECODE set -- is MGH_ERR_INVALID_ARGUMENT before anything is
 * launched, and the context stays usable. */
int mgh_lossless_decompress_sym16(mgh_lossless_ctx *ctx, const uint8_t *payload, uint64_t size, int lossless,
                                  uint16_t *d_symbols, uint64_t n, uint64_t first, uint64_t count,
                                  const uint64_t **d_outlier_idx_out, const int64_t **d_outlier_val_out,
                                  uint64_t *outlier_count_out, void *stream);

/* HOST only (like mgh_infer_level_shape): where the coefficients of `level` lie in a level-linearised
 * (reorder = 1) record -- integers [first_elem, first_elem + num_elems) with first_elem = N_{level-1}
 * (0 for level 0) and N_l = prod(level_shape(l)) -- and the Huffman chunks that hold them, by the
 * header's huff_block_size. Any out pointer may be NULL. Decomposed containers and levels outside
 * 0 ... l_target are refused like mgh_infer_level_shape refuses them. */
int mgh_infer_level_range(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                          int level, uint64_t *first_elem, uint64_t *num_elems, uint64_t *first_chunk,
                          uint64_t *num_chunks);

/* ---- Progressive reader (EXTENSION; DataRefactor::Recompose(data, start_level, stop_level, queue),
 * DataRefactor.hpp:108-124, is the reference's notion of a partial walk): a coarse level now, finer
 * ones when they are wanted, without starting over.
 * open: parses and validates the head once, uploads decode tables, chunk table and outlier lists once
 * (a Huffman_Zstd frame is inflated once; a RAW record is turned into its level-linearised integers
 * once, by the route of mgh_decompress_level). The container is BORROWED: the caller keeps it alive
 * and unchanged until close. Host and device containers as for mgh_decompress. Needs a container with
 * ONE subdomain (else MGH_ERR_INVALID_ARGUMENT, as mgh_decompress_level) written with reorder = 1
 * (else MGH_ERR_INVALID_ARGUMENT: the levels of a reorder = 0 record are spread over every chunk).
 * refine: to_level must be ABOVE mgh_progressive_level (-1 before the first call), else
 * MGH_ERR_INVALID_ARGUMENT. Decodes only chunks not decoded before (the tail of a boundary chunk stays
 * on the device: every chunk is decoded at most once over any sequence of calls), runs
 * mgh_refine_level per level (the first call: mgh_dequantize_recompose_linear_to_level) and returns
 * the dense array of to_level like mgh_decompress_level returns it (in the container's memory space,
 * or in the caller's buffer). Bit-identical to mgh_decompress_level(to_level); at l_target to
 * mgh_decompress. The nodal array of the current level stays on the device as the state.
 * mgh_last_decompress_stats reports each refine's own chunks. */
typedef struct mgh_progressive mgh_progressive;
int mgh_progressive_open(mgh_progressive **out, const void *compressed_data, size_t compressed_size,
                         const mgh_config *config);
int mgh_progressive_level(const mgh_progressive *p);
int mgh_progressive_refine(mgh_progressive *p, int to_level, void **data, int output_pre_allocated);
/* The reader's current level prolonged to the full grid (mgh_prolong): an array of the container's
 * shape, in the container's memory space or in the caller's buffer. Equal to
 * mgh_decompress_preview(l_target - level). Needs one refine before it; does not change the reader's
 * state -- a later refine gives what it would have given. */
int mgh_progressive_preview(mgh_progressive *p, void **data, int output_pre_allocated);
/* ... the box [lo_d, lo_d + ext_d) of it (mgh_prolong_window): a dense array of shape ext, bit for bit
 * the crop of mgh_progressive_preview. The reader's state is untouched. */
int mgh_progressive_preview_window(mgh_progressive *p, const uint64_t *lo, const uint64_t *ext, void **data,
                                   int output_pre_allocated);
void mgh_progressive_close(mgh_progressive *p);

/* ---- Reader of precision layers (EXTENSION; the containers of mgh_compress_layers) -------------------
 * A handle keeps the coefficients of the array, as the layers added so far give them, on the device
 * (one array of the data's type). open takes layer 0, add the NEXT layer -- the containers carry no
 * index, the order is the caller's -- and each costs a decode and one stream over the coefficients
 * (mgh_dequantize_add); nothing is recomposed until mgh_layers_data, which runs mgh_recompose into an
 * array in the memory space of layer 0's container, or into the caller's buffer, and leaves the handle as
 * it was: more layers may follow. The containers are not kept: they may go away when the call returns.
 * add refuses with MGH_ERR_INVALID_ARGUMENT, and leaves the handle as it was, a container whose shape,
 * data type, coordinates, bound type, s, header norm or decomposition are not layer 0's, whose tolerance
 * is not below the last layer's, whose record is RAW, that was written with reorder = 1 or that has more
 * than one subdomain (open refuses the last three). count: layers added (-1 for NULL); tolerance: the
 * last layer's (the header's). mgh_decompress_layers is open, add ... add, data, close in one call;
 * nlayers in 1..64. After one layer the data is mgh_decompress's of that container, bit for bit. */
typedef struct mgh_layers mgh_layers;
int mgh_layers_open(mgh_layers **out, const void *compressed_data, size_t compressed_size, const mgh_config *config);
int mgh_layers_add(mgh_layers *p, const void *compressed_data, size_t compressed_size);
int mgh_layers_count(const mgh_layers *p);
double mgh_layers_tolerance(const mgh_layers *p);
int mgh_layers_data(mgh_layers *p, void **data, int output_pre_allocated);
void mgh_layers_close(mgh_layers *p);
int mgh_decompress_layers(int nlayers, const void *const *compressed_data /* [nlayers] */,
                          const size_t *compressed_size /* [nlayers] */, const mgh_config *config,
                          void **decompressed_data, int output_pre_allocated);
/* The coefficients the handle holds recomposed to `level` (0 .. l_target) only: mgh_recompose_to_level of
 * the accumulator, the dense array of level_shape(level), placed as mgh_layers_data places its output. No
 * fewer bytes were read for it (the layers are reorder = 0 records); it answers the question
 * mgh_level_layers_data answers. */
int mgh_layers_data_level(mgh_layers *p, int level, void **data, int output_pre_allocated);

/* ---- Reader of precision layers in level order (EXTENSION; the containers of mgh_compress_level_layers) --
 * A handle keeps the coefficients in LEVEL-LINEARISED order on the device (one array of the data's type), a
 * decode buffer sized by the largest window decoded so far, and per layer its header and its DEPTH: the
 * level up to which it has been added. With N_l = prod(level_shape(l)):
 *   open(buf0, level)      layer 0 up to `level`: the ceil(N_level / huff_block_size) leading chunks of its
 *                          record are decoded, the window [0, N_level) is stored.
 *   add(buf, level)        the NEXT layer, level <= depth of the last one: a prefix decode, added.
 *   extend(k, buf, level)  layer k deeper: depth[k] < level, and level <= depth[k - 1] for k > 0. Decodes
 *                          from the chunk that holds N_depth[k] (that boundary chunk may be decoded a second
 *                          time, nothing else is); the window [N_depth[k], N_level) is stored for k == 0 and
 *                          added otherwise. The container must be the one recorded for layer k (header,
 *                          tolerance, dictionary and chunk size).
 *   data(level)            level <= depth[0]: mgh_recompose_linear_to_level of the head [0, N_level) into
 *                          an array of level_shape(level) in the memory space of layer 0's container, or
 *                          the caller's buffer. The handle stays as it was.
 * Depths are non-increasing in k: a finer layer alone on a level would be a residual with nothing under
 * it, so on every level the coefficients are the sum of a leading run of layers. MGH_ERR_INVALID_ARGUMENT,
 * with the handle unchanged and before the coefficients are touched: a reorder = 0 container, a
 * domain-decomposed one, a RAW record, a header that is not layer 0's (shape, data type, coordinates,
 * bound type, s, norm), a tolerance that is not below the last layer's, a level outside the rules above.
 * count (-1 for NULL), depth(k) (-1 for a bad k), tolerance(k) (0 for a bad k). The containers are not
 * kept. mgh_last_decompress_stats: the chunks decoded and bytes moved by the last open / add / extend.
 * mgh_decompress_level_layers: open, add ... add, data, close with every layer at `level`; nlayers 1..64. */
typedef struct mgh_level_layers mgh_level_layers;
int mgh_level_layers_open(mgh_level_layers **out, const void *compressed_data, size_t compressed_size,
                          const mgh_config *config, int level);
int mgh_level_layers_add(mgh_level_layers *p, const void *compressed_data, size_t compressed_size, int level);
int mgh_level_layers_extend(mgh_level_layers *p, int k, const void *compressed_data, size_t compressed_size, int level);
int mgh_level_layers_count(const mgh_level_layers *p);
int mgh_level_layers_depth(const mgh_level_layers *p, int k);
double mgh_level_layers_tolerance(const mgh_level_layers *p, int k);
int mgh_level_layers_data(mgh_level_layers *p, int level, void **data, int output_pre_allocated);
void mgh_level_layers_close(mgh_level_layers *p);
int mgh_decompress_level_layers(int nlayers, const void *const *compressed_data /* [nlayers] */,
                                const size_t *compressed_size /* [nlayers] */, int level, const mgh_config *config,
                                void **decompressed_data, int output_pre_allocated);

/* ---- Arrays with missing values (EXTENSION; mgh_mask_* of mgard_hip.h) -------------------------------
 * mgh_compress of an array whose NaN / +-Inf (MGH_MASK_NONFINITE) and / or whose elements equal to
 * (T)fill_value (MGH_MASK_VALUE) do not count: scan -> c = (T)(0.5 vmin + 0.5 vmax), evaluated in double
 * -> fill (mgh_mask_fill's rule) -> mgh_compress of the filled device array, with tol, s, the bound type,
 * coords and config (its domain decomposition included) passed through unchanged -> mask record -> footer:
 *   [ordinary container, C bytes][mask record, R bytes][48-byte footer]      (csrc/mask_plan.hpp)
 * The first C bytes ARE the container mgh_compress writes for the filled array: every reader opens them
 * without knowing about masks (stock MGARD-X, mgh_decompress_level, previews, the progressive reader,
 * mgh_verify against the filled array). The footer is found from the end of the buffer.
 * The error bound holds at every VALID position: valid elements enter the writer unchanged. The header's
 * norm (REL) is the FILLED array's, because the header must describe the array the container holds: for
 * s = inf it equals the absmax of the valid elements exactly (fills are copies of valid values or lie
 * between vmin and vmax); for finite s it includes the filled points.
 * Input: a host array (uploaded once, filled in place on the device) or a device array (filled into one
 * temporary of the array's size). If the array plus that temporary do not fit config->max_memory_footprint
 * the call is MGH_ERR_INVALID_ARGUMENT: masked arrays that must be streamed in parts are not supported.
 * 1 ... 2^32 - 1 elements. The output lands in the input's memory space, allocated like mgh_compress's
 * (plus the packed mask and the footer); MGH_ERR_OUTPUT_TOO_LARGE when a pre-allocated output cannot hold
 * container + record + footer. Every masked position decodes to restore_value: +Inf and NaN are not told
 * apart after the round trip. */
typedef struct mgh_mask_spec {
  int flags;            /* MGH_MASK_NONFINITE | MGH_MASK_VALUE */
  double fill_value;    /* read with MGH_MASK_VALUE */
  double restore_value; /* what mgh_decompress_masked stores at masked positions; may be NaN */
} mgh_mask_spec;
int mgh_compress_masked(int D, int dtype, const uint64_t *shape, double tol, double s, int error_bound_type,
                        const void *original_data, const mgh_mask_spec *spec, void **compressed_data,
                        size_t *compressed_size, const void *const *coords, const mgh_config *config,
                        int output_pre_allocated);

/* 1 and *info for a masked buffer, 0 for a buffer without the footer's magic, MGH_ERR_FORMAT for a footer
 * that has the magic and fails a check (C + R + 48 == size, R against kind and against the n of the
 * container's header, the record's CRC-32). Host work; of a device buffer the footer, the header and the
 * record are copied first. kind: 0 packed words, 1 one record of the lossless stage, 2 nothing masked. */
struct mgh_masked_info { /* (the tag only: the function has the name) */
  uint64_t container_size, record_size, n_masked;
  int kind;
  double restore_value;
};
int mgh_masked_info(const void *compressed_data, size_t compressed_size, struct mgh_masked_info *info);

/* mgh_decompress of the first C bytes, then the mask record, then mgh_mask_restore: the array with
 * restore_value's bits at every masked position. Memory-space rules of mgh_decompress. A buffer without
 * the footer is MGH_ERR_FORMAT (plain containers have mgh_decompress). */
int mgh_decompress_masked(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                          void **decompressed_data, int output_pre_allocated);
/* The mask alone: one byte per element, 0 or 1, into `mask` (host or device memory of the caller,
 * n bytes; n from mgh_infer_shape). */
int mgh_decompress_mask(const void *compressed_data, size_t compressed_size, const mgh_config *config, uint8_t *mask);

/* ---- Masked buffers in the reduced-resolution, preview and verify readers ------------------------------
 * THE RULE (part of the contract):
 *  - a node of a level array or of a coarsened array is masked when the element of the FULL array at that
 *    node's index (mgh_infer_level_nodes, mgh_infer_coarsened_nodes) is masked. This is sampling: there is
 *    no "any masked neighbour" rule;
 *  - a position of a preview or of a preview window is masked when that position of the full array is;
 *  - masked positions of any output hold restore_value's bits; every other position holds, bit for bit,
 *    what the same reader writes for the container part (the first C bytes) alone.
 * The container holds the FILLED array, so valid values near masked regions carry the influence of the
 * fill: a coarse node next to land is a coarse node of the filled field. A preview carries no bound anyway.
 * Each call is: the footer -> the plain reader on the first C bytes -> the mask record -> the sample of the
 * packed mask through the node lists (mgh_mask_sample_; the window's lists are lo + i, and only its bits are
 * gathered; the preview uses the full mask) -> mgh_mask_restore. Arguments, refusals and memory-space rules
 * are those of the reader each one wraps (mgh_decompress_masked_level needs one subdomain, like
 * mgh_decompress_level; the coarsened and preview readers take decomposed containers). A buffer without
 * the footer is MGH_ERR_FORMAT. When nothing is masked (kind 2) the output is the plain reader's.
 * Not built: the progressive reader with a mask; masked layers, ladders, budgets and targets; _multi and
 * _dist; telling NaN from Inf. */
int mgh_decompress_masked_level(const void *compressed_data, size_t compressed_size, int level, void **decompressed_data,
                                const mgh_config *config, int output_pre_allocated);
int mgh_decompress_masked_coarsened(const void *compressed_data, size_t compressed_size, int halvings,
                                    void **decompressed_data, const mgh_config *config, int output_pre_allocated);
int mgh_decompress_masked_preview(const void *compressed_data, size_t compressed_size, int halvings,
                                  void **decompressed_data, const mgh_config *config, int output_pre_allocated);
int mgh_decompress_masked_preview_window(const void *compressed_data, size_t compressed_size, int halvings,
                                         const uint64_t *lo, const uint64_t *ext, void **decompressed_data,
                                         const mgh_config *config, int output_pre_allocated);
/* The sampled mask alone, one byte (0 or 1) per element of the level array, of the coarsened array or of the
 * window [lo, lo + ext), into `mask` (host or device memory of the caller), like mgh_decompress_mask. */
int mgh_decompress_mask_level(const void *compressed_data, size_t compressed_size, int level, const mgh_config *config,
                              uint8_t *mask);
int mgh_decompress_mask_coarsened(const void *compressed_data, size_t compressed_size, int halvings,
                                  const mgh_config *config, uint8_t *mask);
int mgh_decompress_mask_window(const void *compressed_data, size_t compressed_size, const uint64_t *lo,
                               const uint64_t *ext, const mgh_config *config, uint8_t *mask);

/* mgh_verify of a masked buffer against the user's OWN array, marks (NaN, +-Inf, fill values) included: it is
 * mgh_verify on the container part with the masked compare kernel (mgh_compare_masked_) in place of the
 * compare kernel -- per subdomain, its box is held against the full array's packed mask where it lies. Masked
 * positions take part in nothing: stats.n counts the valid positions, *n_masked_out (may be NULL) the others.
 * Nothing of the array's size is allocated beyond what mgh_verify allocates, plus the packed mask.
 * The verdict: s = inf -- achieved = max_abs_err over the valid positions against the header's bound; s = 0
 * -- achieved = sqrt(sum_sq_err / N) under normalize_coordinates (sqrt(sum_sq_err) without), N ALL elements
 * of the array, masked ones included: the writer bounds the sum over the whole filled array, of which the
 * valid positions are a part. within = 0 when an unmasked position is not finite. Any other s, and
 * halvings > 0, as in mgh_verify (within = -1). A buffer without the footer is MGH_ERR_FORMAT. */
int mgh_verify_masked(const void *compressed_data, size_t compressed_size, const void *original, size_t original_bytes,
                      int original_dtype, int halvings, const mgh_config *config, mgh_verify_result *out,
                      uint64_t *n_masked_out);

/* ---- Pointwise relative error bound (EXTENSION; the reference has nothing here) -----------------------
 * |x' - x| <= eps |x| at EVERY element, where REL and ABS bound a norm over the whole array: the masked writer
 * around the field y = log2|x|, compressed under an ABS, s = inf bound delta (csrc/pwrel_plan.hpp has the
 * classes, the derivation of delta and the trailer; mgard_hip.h the result types):
 *   forward pass (x is read once: y = (T)log2((double)|x|), the mask = non-finite or |x| < floor_eff, the flag
 *   bits = non-finite or negative, the statistics) -> delta = log2(1 + eps) - ulp_T(max |y|) - 1.5 E2, E2 = 2^-23
 *   (float) / 2^-52 (double) -> fill -> the masked writer on y (restore_value 0) -> flag record -> footer:
 *   [masked buffer of y, M bytes][flag record, S bytes][56-byte footer]
 * The first M bytes ARE what mgh_compress_masked writes for y: mgh_decompress_masked opens them (the filled y with
 * 0 at the masked positions), and their own first C bytes are an ordinary container of the filled y. The last
 * bytes are not the masked footer's magic: mgh_masked_info of the whole buffer returns 0.
 * floor_eff = max(abs_floor, smallest normal of T): +-0, denormals and values below it decode to +0.0; NaN and
 * +-Inf decode to a quiet NaN; every other element keeps its sign and meets the bound.
 * eps must be finite with 0 < eps < 1 and abs_floor finite and >= 0 (MGH_ERR_INVALID_ARGUMENT). Where delta
 * is below 64 ulp_T(max |y|) (the container's own rounding of y, measured: pwrel_plan.hpp) or the roundings of the
 * transform would take more than half of log2(1 + eps) -- float with 64 <= |y| < 128: eps below about 3.5e-4, and
 * 6.9e-4 where the largest finite value puts |y| at 128; double with 512 <= |y| < 1024: below about 5.2e-12 --
 * the call is MGH_ERR_INVALID_ARGUMENT with a message that says so: a looser bound is never delivered silently.
 * coords and config (its domain decomposition included) pass through unchanged. Memory spaces, footprint
 * (a host array is uploaded once and transformed in place; a device array is not modified and y is written beside
 * it), element count and MGH_ERR_OUTPUT_TOO_LARGE as for mgh_compress_masked.
 * Not built: the progressive reader and verify of a view of such buffers; ladders, budgets, targets and layers;
 * _multi and _dist; telling NaN from Inf, or -0.0 from +0.0. */
int mgh_compress_pwrel(int D, int dtype, const uint64_t *shape, double eps, double abs_floor, const void *original_data,
                       void **compressed_data, size_t *compressed_size, const void *const *coords,
                       const mgh_config *config, int output_pre_allocated);
/* The footer -> mgh_decompress of the container part -> mask words and flag words -> the inverse pass: quiet NaN,
 * +0.0, or +-exp2(y') with the magnitude clamped to [smallest normal, largest finite] of T. Memory-space rules of
 * mgh_decompress. A buffer without the footer (a plain container, a masked buffer) is MGH_ERR_FORMAT. */
int mgh_decompress_pwrel(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                         void **decompressed_data, int output_pre_allocated);
/* Such a buffer at reduced resolution and in previews. THE RULE (part of the contract):
 *  - a node of a level array or of a coarsened array takes its CLASS AND SIGN from the element of the FULL array at
 *    that node's index (mgh_infer_level_nodes, mgh_infer_coarsened_nodes). This is sampling, as for masks;
 *  - a position of a preview or of a preview window takes them from that position of the full array;
 *  - the class is read from the mask bit and the flag bit: both -> a quiet NaN; the mask bit alone -> +0.0;
 *    otherwise +-T(exp2((double)y')), where y' is bit for bit what the reader of the same name without `pwrel_`
 *    writes for the container part (the first C bytes) alone, the flag bit is the sign and the magnitude is clamped
 *    to [smallest normal, largest finite] of T: the inverse pass of mgh_decompress_pwrel, unchanged.
 * THE OUTPUT CARRIES NO ERROR BOUND: it is exp2 of a coarse or prolonged y, and near zeroed or non-finite elements it
 * carries the influence of the fill. level = l_target, halvings = 0 and the preview at 0 halvings are bit for bit
 * mgh_decompress_pwrel.
 * Each call is: the footer -> the plain reader on the first C bytes -> the mask record and the flag record of the
 * full array -> one pass over the view that reads both bits through the view's node lists (the window's lists are
 * lo + i; the preview runs the full array's inverse pass). Arguments, refusals and memory-space rules are those of
 * the reader each one wraps, as for the mgh_decompress_masked_* readers (_level needs one subdomain; the coarsened
 * and preview readers take decomposed containers). A buffer without the footer is MGH_ERR_FORMAT.
 * The classes and signs of a view alone are its masks: mgh_decompress_mask_level / _coarsened / _window on the first
 * M bytes (the masked buffer) give the sampled mask bit. */
int mgh_decompress_pwrel_level(const void *compressed_data, size_t compressed_size, int level, void **decompressed_data,
                               const mgh_config *config, int output_pre_allocated);
int mgh_decompress_pwrel_coarsened(const void *compressed_data, size_t compressed_size, int halvings,
                                   void **decompressed_data, const mgh_config *config, int output_pre_allocated);
int mgh_decompress_pwrel_preview(const void *compressed_data, size_t compressed_size, int halvings,
                                 void **decompressed_data, const mgh_config *config, int output_pre_allocated);
int mgh_decompress_pwrel_preview_window(const void *compressed_data, size_t compressed_size, int halvings,
                                        const uint64_t *lo, const uint64_t *ext, void **decompressed_data,
                                        const mgh_config *config, int output_pre_allocated);
/* 1 and *info for such a buffer, 0 for a buffer without the footer's magic, MGH_ERR_FORMAT for a footer that has
 * the magic and fails a check (M + S + 56 == size, the masked buffer's own checks, S against kind and n,
 * n_flag <= n, the flag record's CRC-32). delta is the tolerance in the container's header. Kinds: 0 packed
 * words, 1 one record of the lossless stage, 2 no bit set. */
struct mgh_pwrel_info { /* (the tag only: the function has the name) */
  double eps, abs_floor, delta;
  uint64_t n_masked, n_flag;
  uint64_t container_size, masked_size, mask_record_size, flag_record_size;
  int mask_kind, flag_kind;
};
int mgh_pwrel_info(const void *compressed_data, size_t compressed_size, struct mgh_pwrel_info *info);
/* Decodes the whole array and holds it against the user's OWN array in one pass, with the footer's abs_floor
 * (mgh_pwrel_compare, mgard_hip.h). *within (may be NULL) = 1 exactly when max_rel_err <= eps, there is no class
 * and no sign mismatch, and the largest zeroed |x| lies below floor_eff; 0 otherwise. The original may be a host
 * or a device array of the buffer's type and size (MGH_ERR_INVALID_ARGUMENT otherwise). */
int mgh_verify_pwrel(const void *compressed_data, size_t compressed_size, const void *original, size_t original_bytes,
                     int original_dtype, const mgh_config *config, mgh_pwrel_compare *out, int *within);

/* ---- Region of interest (EXTENSION; the reference has nothing here) ------------------------------------
 * A tighter POINTWISE bound inside up to 16 disjoint boxes of an array, without paying it everywhere
 * (csrc/roi_plan.hpp has the rules of the boxes, the derivation of the bound and the trailer):
 *   C0 = mgh_compress(x, tol), unchanged -> b = mgh_decompress(C0) on the device -> per box one pass: the dense
 *   residual r_i = fl_T(x[box_i] - b[box_i]) with max |r_i|, max |x| and the count of non-finite values -> tolres_i
 *   -> C_i = mgh_compress(r_i): ABS, s = inf, shape ext_i, no coordinates, the caller's lossless and huff_block_size
 *   -> [C0][C_0] ... [C_{nbox-1}][box table, 120 nbox bytes][40-byte footer]
 * The first C bytes ARE what mgh_compress(x, tol) writes (that call writes them; two calls agree byte for byte up to
 * the order of the outlier pairs inside a record): every plain reader opens them as the unrefined base.
 * With A = tol (ABS) or tol * the norm in C0's header (REL), and A_i = tol_i times the same factor, the decoded
 * array is within A_i of x at every element of box i and within A everywhere:
 *   |x'' - x| <= |r_i' - r_i| + ulp_T(max |r_i|) / 2 + ulp_T(max |x| + A_i) / 2, so
 *   tolres_i = A_i - ulp_T(max |r_i|) / 2 - ulp_T(max |x| + A_i) / 2.
 * Outside the boxes the output is bit for bit mgh_decompress of the first C bytes.
 * MGH_ERR_INVALID_ARGUMENT, with a message: s not infinite (any other s bounds a norm, not a point); nbox outside
 * 1 .. 16; a box that leaves the array, has an extent below 3 or meets another box; tol_i outside (0, tol); 2^32
 * elements or more; an array that, with its decoded base beside it, does not fit max_memory_footprint (arrays with
 * boxes are not streamed in parts); a non-finite value in a box (masked arrays with boxes are not built); and where
 * tolres_i < A_i / 2 or tolres_i < 64 ulp_T(max |r_i|) -- the data type cannot carry tol_i there (the 64 ulps are
 * the measured limit of the container path: pwrel_plan.hpp): a looser bound is never delivered silently.
 * A box in which the base is exact (max |r_i| = 0) stores nothing: record size 0.
 * coords and config pass through to C0 unchanged (it may be domain-decomposed). Memory spaces and
 * MGH_ERR_OUTPUT_TOO_LARGE as for mgh_compress_masked. */
typedef struct mgh_roi_box {
  uint64_t lo[MGH_MAX_DIM], ext[MGH_MAX_DIM]; /* the first D entries of each */
  double tol;
} mgh_roi_box;
int mgh_compress_roi(int D, int dtype, const uint64_t *shape, double tol, double s, int error_bound_type,
                     const void *original_data, int nbox, const mgh_roi_box *boxes, void **compressed_data,
                     size_t *compressed_size, const void *const *coords, const mgh_config *config,
                     int output_pre_allocated);
/* The footer and the table -> mgh_decompress of the first C bytes -> per box with a record: mgh_decompress of C_i
 * into a device buffer and out[box_i] = fl_T(out[box_i] + r_i') in place. Memory-space rules of mgh_decompress.
 * A buffer without the footer (a plain container, a masked or pointwise-relative buffer) is MGH_ERR_FORMAT. */
int mgh_decompress_roi(const void *compressed_data, size_t compressed_size, void **decompressed_data,
                       const mgh_config *config, int output_pre_allocated);
/* 1 and *info for such a buffer, 0 for a buffer without the footer's magic, MGH_ERR_FORMAT for a footer that has
 * the magic and fails a check (every size and offset against the buffer, the table's and the records' CRC-32, the
 * boxes against the shape in C0's header). D is the array's; lo and ext hold D entries. */
struct mgh_roi_info { /* (the tag only: the function has the name) */
  uint64_t container_size;
  int nbox, D;
  struct {
    uint64_t lo[MGH_MAX_DIM], ext[MGH_MAX_DIM];
    double tol, tolres;
    uint64_t record_size;
  } box[16];
};
int mgh_roi_info(const void *compressed_data, size_t compressed_size, struct mgh_roi_info *info);
/* Decodes the whole array into a device buffer and holds it against the user's OWN array with mgh_compare's
 * reduction: *whole over the entire array against A (which, since A_i < A, covers the outside of the boxes), and
 * per_box[i] (nbox entries; may be NULL) over box i, through the array's leading dimensions, against A_i;
 * argmax is then the flat index inside the box. bound_kind = 0; within = 1 exactly when nothing is non-finite and
 * max_abs_err <= bound. The original may be a host or a device array of the buffer's type and size. */
int mgh_verify_roi(const void *compressed_data, size_t compressed_size, const void *original, size_t original_bytes,
                   int original_dtype, const mgh_config *config, mgh_verify_result *whole, mgh_verify_result *per_box);

#ifdef __cplusplus
}
#endif
#endif /* MGARD_HIP_COMPRESS_H */
