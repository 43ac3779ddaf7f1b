/*
 * mgard_hip.h -- C ABI of the MI355X-native MGARD-X hot path
 * (multilevel decomposition chain + level-wise linear quantizer).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point names the reference (CODARcode/MGARD v1.6.0) interface it
 * replaces; paths are relative to the reference checkout.
 *
 * Conventions
 *  - All data pointers are DEVICE pointers on the hierarchy's device unless the
 *    parameter name starts with h_ (host).
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream). Calls
 *    are asynchronous with respect to the host unless stated otherwise.
 *  - Arrays are dense row-major with the LAST dimension fastest, shape given at
 *    hierarchy creation (mgard_x convention, shape[D-1] = fastest).
 *  - Return value: MGH_SUCCESS (0) or a negative mgh_status. No exceptions
 *    cross this boundary. mgh_last_error() gives a human-readable message.
 */
#ifndef MGARD_HIP_H
#define MGARD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mgh_status {
  MGH_SUCCESS = 0,
  MGH_ERR_INVALID_ARGUMENT = -1,
  MGH_ERR_UNSUPPORTED_DIMENSION = -2, /* cf. NotSupportHigherNumberOfDimensionsFailure */
  MGH_ERR_UNSUPPORTED_DTYPE = -3,     /* cf. NotSupportDataTypeFailure */
  MGH_ERR_DEVICE = -4,                /* HIP runtime error (message in mgh_last_error) */
  MGH_ERR_OUT_OF_MEMORY = -5,
  MGH_ERR_NO_DEVICE = -6 /* cf. BackendNotAvailableFailure */
} mgh_status;

/* mgard_x::data_type (include/mgard-x/Utilities/Types.h:41) */
typedef enum mgh_dtype { MGH_FLOAT = 0, MGH_DOUBLE = 1 } mgh_dtype;
/* mgard_x::error_bound_type (include/mgard-x/Utilities/Types.h:32) */
typedef enum mgh_error_bound { MGH_REL = 0, MGH_ABS = 1 } mgh_error_bound;

#define MGH_MAX_DIM 5

/* Opaque handle: level shapes + per-level spacing tables on host and device,
 * plus the device workspace the kernels need. Replaces
 * mgard_x::Hierarchy<D,T,HIP> (include/mgard-x/Hierarchy/Hierarchy.hpp:193-418,
 * ctor :712-757) together with the workspace half of
 * mgard_x::DataRefactor<D,T,HIP> (include/mgard-x/DataRefactoring/DataRefactor.hpp:19-71). */
typedef struct mgh_hierarchy mgh_hierarchy;

const char *mgh_last_error(void);
/* Number of visible HIP devices (0 if none / no driver). */
int mgh_device_count(void);

/* h_coords: NULL for a uniform grid (Hierarchy(shape, config), Hierarchy.hpp:712),
 * else D host arrays of `dtype` with shape[d] strictly increasing coordinates
 * (Hierarchy(shape, coords, config), Hierarchy.hpp:741). normalize_coordinates
 * mirrors Config::normalize_coordinates (Config/Config.h:22), max_level mirrors
 * Config::max_larget_level (pass UINT64_MAX for "no limit"). */
int mgh_hierarchy_create(mgh_hierarchy **out, int D, const uint64_t *shape, int dtype,
                         const void *const *h_coords, int normalize_coordinates,
                         uint64_t max_level, int device);
void mgh_hierarchy_destroy(mgh_hierarchy *h);

int mgh_l_target(const mgh_hierarchy *h);                       /* Hierarchy::l_target() */
int mgh_level_shape(const mgh_hierarchy *h, int level, uint64_t *out_shape); /* ::level_shape(l) */
uint64_t mgh_total_num_elems(const mgh_hierarchy *h);           /* ::total_num_elems() */
/* Device bytes held by the handle (tables + workspace). */
size_t mgh_device_bytes(const mgh_hierarchy *h);
/* Device address of the norm (one value of the hierarchy's type) the last fused call with a REL
 * bound and no host read-back (h_norm_out == NULL) computed and used; valid until the next call on
 * the handle. Lets a caller fetch the norm with its own asynchronous copy behind later work instead
 * of paying a synchronisation inside mgh_decompose_quantize*. NULL for a NULL handle. */
const void *mgh_norm_device_ptr(const mgh_hierarchy *h);

/* Host copies of the per-level tables, for inspection/tests. kind: 0=dist
 * (Hierarchy::dist), 1=ratio (::ratio), 2=am, 3=bm (n+1 entries, ::am/::bm),
 * 4=level_marks (int32, only level == l_target). Returns the number of entries
 * written to h_out (capacity `cap` entries), or a negative status. */
int64_t mgh_hierarchy_table(const mgh_hierarchy *h, int kind, int level, int dim, void *h_out,
                            uint64_t cap);

/* Norm used for REL error bounds. Replaces Compressor::CalculateNorm ->
 * norm_calculator (include/mgard-x/CompressionLowLevel/NormCalculator.hpp:12-80).
 * s = +inf: max|x|; otherwise sqrt(sum x^2 / N) (normalize_coordinates) or
 * sqrt(sum x^2); 0 -> epsilon. SYNCHRONOUS (returns the value to the host). */
int mgh_norm(mgh_hierarchy *h, const void *d_data, double s, double *h_norm_out, void *stream);

/* Multilevel decomposition. Replaces Compressor::Decompose ->
 * DataRefactor::Decompose -> multi_dimension::decompose
 * (include/mgard-x/DataRefactoring/MultiDimension/DataRefactoring.hpp:25-177).
 * d_coeff receives the coefficients in MGARD-X's in-place reordered layout
 * (coarse corner first, level by level). d_coeff may equal d_data (the
 * reference's in-place behaviour; costs one extra copy here). */
int mgh_decompose(mgh_hierarchy *h, const void *d_data, void *d_coeff, void *stream);

/* Inverse. Replaces Compressor::Recompose -> multi_dimension::recompose
 * (DataRefactoring.hpp:179-317). d_data may equal d_coeff. */
int mgh_recompose(mgh_hierarchy *h, const void *d_coeff, void *d_data, void *stream);

/* Level-wise linear quantizer. Replaces Compressor::Quantize ->
 * LinearQuantizer::Quantize (include/mgard-x/Quantization/LinearQuantization.hpp
 * :564-683; quantizers :495-545; kernel :21-301). Output keeps the reordered N-D
 * layout (config.reorder == 0). With prep_huffman != 0 values are shifted by
 * dict_size/2 and values outside [0, dict_size) go to the outlier list
 * (linear index, shifted value) while 0 is stored in d_quantized (:208-241).
 * d_outlier_count is a single uint64 on the device, zeroed by this call; if it
 * ends up larger than outlier_capacity only the first outlier_capacity entries
 * were stored and the caller must retry with bigger buffers (:621-676).
 * Outlier order is unspecified (atomic order), as in the reference. */
int mgh_quantize(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol,
                 double s, double norm, uint64_t dict_size, int prep_huffman,
                 int64_t *d_quantized, uint64_t *d_outlier_count, uint64_t *d_outlier_idx,
                 int64_t *d_outlier_val, uint64_t outlier_capacity, void *stream);

/* Replaces Compressor::Dequantize -> LinearQuantizer::Dequantize
 * (LinearQuantization.hpp:685-780, OutlierRestore :304-350). d_quantized is
 * modified (outliers scattered back), like the reference. */
int mgh_dequantize(mgh_hierarchy *h, int64_t *d_quantized, int error_bound_type, double tol,
                   double s, double norm, uint64_t dict_size, int prep_huffman,
                   const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                   uint64_t outlier_count, void *d_coeff, void *stream);

/* The fused hot path: [norm] + decompose + quantize in one call, what
 * Compressor::Compress runs before the lossless stage
 * (include/mgard-x/CompressionLowLevel/Compressor.hpp:193-237, lines 216-218).
 * Coefficients are quantized as they are produced; the float coefficient array
 * is not materialised unless d_coeff_opt != NULL. For REL bounds pass
 * norm <= 0 to have the norm computed here (returned through h_norm_out if not
 * NULL; this makes the call synchronise once), or a positive norm to use it.
 * Results are identical to mgh_decompose followed by mgh_quantize. */
int mgh_decompose_quantize(mgh_hierarchy *h, const void *d_data, int error_bound_type,
                           double tol, double s, double norm, double *h_norm_out,
                           uint64_t dict_size, int prep_huffman, int64_t *d_quantized,
                           uint64_t *d_outlier_count, uint64_t *d_outlier_idx,
                           int64_t *d_outlier_val, uint64_t outlier_capacity,
                           void *d_coeff_opt, void *stream);

/* The same with the quantized values delivered as 16-bit DICTIONARY SYMBOLS (what the lossless
 * stage consumes: q + dict_size/2 in [0, dict_size), out-of-dictionary values as symbol 0 plus an
 * entry of the outlier list, LinearQuantization.hpp:208-241) -- the values of
 * mgh_decompose_quantize(..., prep_huffman = 1, ...) narrowed to uint16_t, a quarter of the
 * output bytes. An extension for callers that feed the Huffman stage directly (mgh_compress does);
 * the reference always materialises the int64 array (QUANTIZED_INT, RuntimeX/DataTypes.h:128).
 * dict_size <= 65536. Only where the fused kernels run (3-D, at least one level), else
 * MGH_ERR_UNSUPPORTED_DIMENSION: use mgh_decompose_quantize there. */
int mgh_decompose_quantize_sym16(mgh_hierarchy *h, const void *d_data, int error_bound_type,
                                 double tol, double s, double norm, double *h_norm_out,
                                 uint64_t dict_size, uint16_t *d_symbols,
                                 uint64_t *d_outlier_count, uint64_t *d_outlier_idx,
                                 int64_t *d_outlier_val, uint64_t outlier_capacity, void *stream);

/* Inverse of mgh_decompose_quantize_sym16: dequantize + recompose from 16-bit symbols and the
 * outlier list (found by index through a hash table: symbol 0 at an outlier's position).
 * Same result as mgh_dequantize_recompose on the widened values. mgh_sym16_supported tells
 * whether this hierarchy runs BOTH *_sym16 calls (1: the fused 3-D path) or not (0); the
 * compression-side call alone also runs on the fused 4-D path and returns
 * MGH_ERR_UNSUPPORTED_DIMENSION elsewhere. */
int mgh_dequantize_recompose_sym16(mgh_hierarchy *h, const uint16_t *d_symbols, int error_bound_type,
                                   double tol, double s, double norm, uint64_t dict_size,
                                   const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                                   uint64_t outlier_count, void *d_data_out, void *stream);
int mgh_sym16_supported(const mgh_hierarchy *h);

/* Leading dimensions of the caller's arrays of the hierarchy's data type (mgard_x::Array::ld,
 * RuntimeX/DataStructures/Array.hpp:70-84: the reference's HIP backend allocates its arrays
 * with hipMallocPitch by default, which pads the FASTEST dimension; SubArray.hpp:136-139
 * carries one ld per dimension). `ld`: D entries, ld[d] >= shape[d] for d >= 1 (ld[0] is not
 * used); element (i0, .., i_{D-1}) lies at ((i0 * ld[1] + i1) * ld[2] + ...) + i_{D-1}.
 * NULL = dense again. which = MGH_LD_IN: every T array an entry point READS (data of
 * mgh_norm*, mgh_decompose, mgh_decompose_quantize*; coefficients of mgh_recompose,
 * mgh_quantize); MGH_LD_OUT: every T array it WRITES (coefficients of mgh_decompose,
 * mgh_dequantize, d_coeff_opt; data of mgh_recompose, mgh_dequantize_recompose*). The
 * quantized integers, symbols and outlier indices are always dense (Compressor.hpp:48-53
 * allocates them unpitched: they are linearised for the lossless stage). The setting stays
 * until it is changed. The fused 3-D kernels read / write the pitched array in place; the
 * other paths (D != 3, thin shapes, stand-alone stages) go through a dense copy inside the
 * hierarchy. mgh_norm_stream_add takes parts of a dense array only. */
#define MGH_LD_IN 0
#define MGH_LD_OUT 1
int mgh_set_ld(mgh_hierarchy *h, int which, const uint64_t *ld);

/* Norm of an input that is still ARRIVING (host -> device in slabs): _begin once, _add
 * for every part that has landed (any partition of the array; `cold` != 0: the part is
 * read with nontemporal loads, for parts the level pass will not find in the cache
 * anyway), then ONE call of mgh_decompose_quantize / mgh_decompose_quantize_sym16 with
 * a REL bound and norm = 0 on the same hierarchy, which takes the accumulated value
 * instead of reducing the array again. max|x| is exact in any order; the L2 sum has
 * the order dependence of its last bits that the one-pass reduction has too. All calls
 * ASYNCHRONOUS, in stream order. Fused 3-D / 4-D path only
 * (MGH_ERR_UNSUPPORTED_DIMENSION elsewhere). No reference counterpart: the reference
 * computes the norm after the whole subdomain has arrived (Compressor.hpp:158-176). */
int mgh_norm_stream_begin(mgh_hierarchy *h, void *stream);
int mgh_norm_stream_add(mgh_hierarchy *h, const void *d_part, uint64_t count, double s, int cold,
                        void *stream);
/* Instead of that one call: ends the accumulation and hands the norm back, converted exactly as the
 * fused call would have converted it (so a later call that is GIVEN this norm quantizes with the same
 * table). Synchronises the stream. */
int mgh_norm_stream_end(mgh_hierarchy *h, double s, double *h_norm_out, void *stream);

/* Histograms of the symbols mgh_quantize(..., prep_huffman = 1) would store, for `ntol` (1..64)
 * tolerances at once, from ONE coefficient array (what mgh_decompose wrote; MGH_LD_IN applies as in
 * mgh_quantize): d_freq[k * dict_size + q] counts the elements whose symbol at tols[k] is q, outliers
 * counted in bin 0 (the quantizer stores 0 for them) and in d_outliers[k]. Both device arrays are
 * zeroed by the call. The level quantizers of every tolerance are the ones mgh_quantize builds.
 * 32-bit counters: arrays of 2^32 elements and more are refused (MGH_ERR_INVALID_ARGUMENT), as are
 * dict_size outside 2..16384. ASYNCHRONOUS behind the upload of the quantizer tables. No reference
 * counterpart. */
int mgh_quantize_histograms(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, int ntol,
                            const double *tols, double s, double norm, uint64_t dict_size,
                            uint32_t *d_freq /* [ntol][dict_size] */, uint64_t *d_outliers /* [ntol] */,
                            void *stream);

/* What the decoder will see of ONE coefficient array at a tolerance, without the integers, the outlier
 * lists or the lossless stage: d_coeff_out[i] is, bit for bit, what mgh_dequantize writes for the
 * integers mgh_quantize makes from d_coeff[i] -- for either prep_huffman and any dict_size (the
 * dictionary shift cancels in int64, and an out-of-dictionary value travels through the outlier list as
 * the same int64, so neither is an argument). The tables are the ones those two calls build, the
 * arithmetic is their kernels' own. MGH_LD_IN applies to d_coeff as in mgh_quantize; d_coeff_out is
 * DENSE (MGH_LD_OUT is not honoured) and may be d_coeff (in place) when that is dense. One read and one
 * write per element. Arrays of 2^32 elements and more are refused (MGH_ERR_INVALID_ARGUMENT; 32-bit index
 * arithmetic, as in mgh_quantize_histograms). ASYNCHRONOUS behind the upload of the quantizer tables. No
 * reference counterpart. */
int mgh_quantize_roundtrip(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol,
                           double s, double norm, void *d_coeff_out, void *stream);

/* ONE coefficient array (what mgh_decompose wrote; MGH_LD_IN applies as in mgh_quantize_roundtrip: a
 * pitched array goes through a dense copy inside the hierarchy) to what the lossless stage reads, in one
 * pass: d_symbols[i] (dense, uint16) is the integer mgh_quantize(..., prep_huffman = 1) stores at i, which
 * lies in [0, dict_size) or is 0 at an outlier's position; the outlier list holds (linear index, the int64
 * mgh_quantize puts into its list) in no particular order. The counter goes on counting past
 * outlier_capacity and nothing is written past it, so a caller learns the size it needs, as with
 * mgh_quantize. d_freq_or_null, when given, receives the histogram of the stored symbols (dict_size
 * 32-bit bins, an outlier counted in bin 0): what a histogram pass over d_symbols would count.
 * THE CALLER ZEROES d_freq_or_null AND *d_outlier_count (in stream order before the call): the call adds
 * to both. The level quantizers are the ones mgh_quantize builds, by the same host code and upload. Every
 * shape the stand-alone quantizer takes, 1-D to 5-D. Refused with MGH_ERR_INVALID_ARGUMENT: dict_size
 * odd or outside 2..16384, NULL d_symbols or d_outlier_count, outlier_capacity > 0 with a NULL list, arrays
 * of 2^32 elements and more (32-bit index arithmetic and counters, as in mgh_quantize_histograms).
 * ASYNCHRONOUS behind the upload of the quantizer table. No reference counterpart. */
int mgh_quantize_symbols(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, double s,
                         double norm, uint64_t dict_size, uint16_t *d_symbols, uint32_t *d_freq_or_null,
                         uint64_t *d_outlier_count, uint64_t *d_outlier_idx, int64_t *d_outlier_val,
                         uint64_t outlier_capacity, void *stream);

/* mgh_quantize_symbols with one more output (precision layers): everything
 * mgh_quantize_symbols writes, for the same arguments and on the same terms (the caller zeroes the bins and
 * the counter, the refusals, MGH_LD_IN), and in addition
 *   d_residual_out[i] = d_coeff[i] - (what mgh_dequantize writes at i for these integers and this bound),
 * bit for bit: the dequantizer's own expression on its own tables, then one IEEE subtraction. At an
 * outlier's position the integer is the one in the list, not the symbol 0 stored in its place.
 * d_residual_out is DENSE (MGH_LD_OUT is not honoured), of the hierarchy's type, never NULL, and may be
 * d_coeff (in place) when that is dense. Quantizing d_residual_out at a smaller tolerance gives the next
 * layer. ASYNCHRONOUS behind the upload of the quantizer tables. No reference counterpart. */
int mgh_quantize_symbols_residual(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, double s,
                                  double norm, uint64_t dict_size, uint16_t *d_symbols, uint32_t *d_freq_or_null,
                                  uint64_t *d_outlier_count, uint64_t *d_outlier_idx, int64_t *d_outlier_val,
                                  uint64_t outlier_capacity, void *d_residual_out, void *stream);

/* The reader's side of it: d_coeff_inout[i] = (first ? nothing : d_coeff_inout[i]) + what mgh_dequantize
 * writes at i for d_quantized, the outlier list and this bound -- `first` STORES that value (bit for bit
 * mgh_dequantize's output), otherwise it is added with one IEEE addition. d_quantized is int64 (a 16-bit
 * symbol input is not taken); like mgh_dequantize the call writes the outliers back into it first, so it
 * is modified. d_coeff_inout is DENSE (MGH_LD_OUT is not honoured). Arrays of 2^32 elements and more are
 * refused (MGH_ERR_INVALID_ARGUMENT). ASYNCHRONOUS behind the upload of the quantizer table. */
int mgh_dequantize_add(mgh_hierarchy *h, int64_t *d_quantized, int error_bound_type, double tol, double s,
                       double norm, uint64_t dict_size, int prep_huffman, const uint64_t *d_outlier_idx,
                       const int64_t *d_outlier_val, uint64_t outlier_count, int first, void *d_coeff_inout,
                       void *stream);

/* Norm that stays on the device: writes one value of the hierarchy's dtype to
 * d_norm_out (max|x| for s = +inf, else the L2 norm of this array as
 * norm_calculator defines it). ASYNCHRONOUS. For a decomposed domain the caller
 * reduces the per-subdomain values itself (MAX for s = +inf; RCCL all-reduce). */
int mgh_norm_device(mgh_hierarchy *h, const void *d_data, double s, void *d_norm_out,
                    void *stream);

/* Fused hot path for one subdomain of a decomposed domain, fully asynchronous:
 * d_norm = GLOBAL norm (dtype of the hierarchy, on the device). The bound applied
 * is the reference's per-subdomain bound, calc_local_abs_tol
 * (include/mgard-x/CompressionHighLevel/ErrorToleranceCalculator.hpp:134-155,
 * applied at CompressionHighLevel.hpp:122-144): REL, s=inf: (T)(tol*norm) as an
 * ABS bound; REL, finite s: sqrt((tol*norm)^2 / num_subdomains); ABS: tol resp.
 * sqrt(tol^2 / num_subdomains). 3-D only. */
int mgh_decompose_quantize_dn(mgh_hierarchy *h, const void *d_data, int error_bound_type,
                              double tol, double s, const void *d_norm, uint64_t num_subdomains,
                              uint64_t dict_size, int prep_huffman, int64_t *d_quantized,
                              uint64_t *d_outlier_count, uint64_t *d_outlier_idx,
                              int64_t *d_outlier_val, uint64_t outlier_capacity, void *stream);

/* Inverse of the above: dequantize + recompose
 * (Compressor::Decompress, Compressor.hpp:239-272, lines 256-257). */
int mgh_dequantize_recompose(mgh_hierarchy *h, int64_t *d_quantized, int error_bound_type,
                             double tol, double s, double norm, uint64_t dict_size,
                             int prep_huffman, const uint64_t *d_outlier_idx,
                             const int64_t *d_outlier_val, uint64_t outlier_count, void *d_data,
                             void *stream);

/* ---- Reconstruction at a coarser level of the hierarchy (reduced resolution) ----------------
 * EXTENSIONS of the compression-level interface: the reference has the operation one layer down,
 * DataRefactor::Recompose(data, start_level, stop_level, queue)
 * (include/mgard-x/DataRefactoring/DataRefactor.hpp:108-124; loop
 * MultiDimension/DataRefactoring.hpp:233,274); these calls fix the range to 0 ... level.
 * Levels are the hierarchy's: 0 = coarsest grid, mgh_l_target(h) = the full array. The result is
 * what the recompose loop holds at the nodes of `level` after the passes l = 1 ... level and none
 * above: the corrected nodal values of that level, written to d_out as a DENSE array of
 * mgh_level_shape(h, level) (MGH_LD_OUT does not apply to these calls; MGH_LD_IN is honoured for
 * d_coeff as mgh_recompose honours it). d_out must not alias the input.
 * d_coeff / d_quantized / d_symbols are the FULL arrays the calls without a level take (full-array
 * strides, outlier indices = positions in the full array). Only the corner box
 * [0, m_0) x ... x [0, m_{D-1}), m = level_shape(level), is read, outliers outside it are ignored,
 * and no work is done that scales with the full array. d_quantized is modified INSIDE the box only
 * (outliers written back), so one buffer serves level 2, then 3, ... then the full call.
 * The quantizers are those of the full hierarchy. level == l_target: the bits of the call without
 * a level; level outside 0 ... l_target: MGH_ERR_INVALID_ARGUMENT, nothing launched. */
int mgh_recompose_to_level(mgh_hierarchy *h, const void *d_coeff, int level, void *d_out, void *stream);
int mgh_dequantize_recompose_to_level(mgh_hierarchy *h, int64_t *d_quantized, int error_bound_type,
                                      double tol, double s, double norm, uint64_t dict_size,
                                      int prep_huffman, const uint64_t *d_outlier_idx,
                                      const int64_t *d_outlier_val, uint64_t outlier_count, int level,
                                      void *d_out, void *stream);
/* (where mgh_sym16_supported(h), like mgh_dequantize_recompose_sym16) */
int mgh_dequantize_recompose_sym16_to_level(mgh_hierarchy *h, const uint16_t *d_symbols,
                                            int error_bound_type, double tol, double s, double norm,
                                            uint64_t dict_size, const uint64_t *d_outlier_idx,
                                            const int64_t *d_outlier_val, uint64_t outlier_count,
                                            int level, void *d_out, void *stream);
/* The same from the HEAD of a level-linearised array (mgh_level_linearize; what a reorder = 1 record
 * holds): its first N_level = prod(level_shape(level)) integers ARE the corner box of `level`, level
 * by level, so nothing behind them is needed.
 * mgh_level_box_from_linear: the permutation on its own -- d_linear [at least N_level] to the compact
 * corner box d_box_out [N_level], reordered layout, dense in level_shape(level); nothing at or behind
 * position N_level is read. level = 0 ... l_target; at l_target the result is
 * mgh_level_linearize(inverse = 1). d_box_out must not be d_linear.
 * mgh_dequantize_recompose_linear_to_level: d_linear holds at least the first N_level integers and no
 * other is read. The outlier indices are LINEARISED positions (as a reorder = 1 record carries them):
 * those at positions >= N_level are skipped, the others are written into d_linear in place before the
 * box is made. d_out is the dense array of level_shape(level), bit-identical to
 * mgh_level_linearize(inverse) + mgh_dequantize_recompose_to_level on the full array. No work scales
 * with the full array; the box buffer is counted in mgh_device_bytes. */
int mgh_level_box_from_linear(mgh_hierarchy *h, const int64_t *d_linear, int level, int64_t *d_box_out,
                              void *stream);
int mgh_dequantize_recompose_linear_to_level(mgh_hierarchy *h, int64_t *d_linear, int error_bound_type,
                                             double tol, double s, double norm, uint64_t dict_size,
                                             int prep_huffman, const uint64_t *d_outlier_idx,
                                             const int64_t *d_outlier_val, uint64_t outlier_count,
                                             int level, void *d_out, void *stream);
/* (The three low-level calls of the precision layers in level order -- mgh_quantize_residual_linear,
 * mgh_dequantize_add_linear, mgh_recompose_linear_to_level -- are declared in mgard_hip_level_layers.h.) */
/* ONE LEVEL STEP of the same loop, for a caller that keeps the result of a coarser level and wants
 * the next one (DataRefactor::Recompose(data, start_level, stop_level, queue) with
 * start_level = level - 1, stop_level = level). level = 1 ... l_target.
 * d_coarse: the dense array of level_shape(level - 1), as a *_to_level call or an earlier
 * mgh_refine_level wrote it; NOT modified (the call works on a copy inside the hierarchy, 1/2^D of the
 * output). d_segment: the N_level - N_{level-1} integers [N_{level-1}, N_level) of the level-linearised
 * array -- the coefficients of that level and nothing else. The outlier indices are linearised
 * positions of the WHOLE array, as above: those inside the segment are written into d_segment in
 * place, all others are skipped. d_out: dense in level_shape(level) (MGH_LD_OUT does not apply); it
 * must alias neither input. Bit-identical to mgh_dequantize_recompose_linear_to_level(level) on the
 * head [0, N_level) of the same array; no work scales with anything but the box of `level`, and none
 * of the levels below is run again. */
int mgh_refine_level(mgh_hierarchy *h, const void *d_coarse, int64_t *d_segment, int error_bound_type,
                     double tol, double s, double norm, uint64_t dict_size, int prep_huffman,
                     const uint64_t *d_outlier_idx, const int64_t *d_outlier_val, uint64_t outlier_count,
                     int level, void *d_out, void *stream);
/* Full-grid preview: the dense array of `level` (level_shape(level), as mgh_recompose_to_level and
 * its siblings write it) prolonged to the hierarchy's own grid. The result is, bit for bit, what
 * mgh_recompose gives for the reordered array that holds d_level in the corner box of `level` and
 * zeros everywhere else: with zero coefficients the load vector, the Thomas solves and the
 * correction are zero, and only the interpolation f, then c, then r of every level above `level`
 * is left. level in 0 ... l_target (else MGH_ERR_INVALID_ARGUMENT, like a NULL pointer);
 * level == l_target is a copy. One exception to "bit for bit", on the kernel route below only: a
 * -0.0 in d_level at a node the finer levels keep is copied, where mgh_recompose subtracts a zero
 * correction that is -0.0 away from the corners of the level and so gives +0.0 -- the sign of a
 * zero, nothing else. d_level is NOT modified. d_out: DENSE in the hierarchy's shape --
 * MGH_LD_OUT is not honoured --, and not d_level.
 * D = 3 on the fused route: one launch of the prolongation kernel per level above `level`, the
 * intermediates in the hierarchy's own level buffers; the only pass of the size of the array is
 * the last launch's streaming write. Every other shape (D <= 2, thin shapes, D = 4, 5,
 * MGH_FORCE_V1, MGH_FORCE_ND): the level loops of mgh_recompose from level + 1 on over an array of
 * zeros -- full-sized work, there so that the call has one meaning on every shape. */
int mgh_prolong(mgh_hierarchy *h, int level, const void *d_level, void *d_out, void *stream);
/* Developer aid: the launch plan of mgh_prolong's kernel for the level step level - 1 -> level
 * (1 ... l_target) as six ints: tile TC, TF (coarse nodes along c, f), tiles along f, tiles of an
 * r-plane, coarse r-planes per workgroup, chunks of the march (the last takes what is left).
 * MGH_ERR_UNSUPPORTED_DIMENSION where mgh_prolong runs no kernel of its own. */
int mgh_debug_prolong_plan(const mgh_hierarchy *h, int level, int *out6);
/* Windowed full-grid preview: the box W = [lo_d, lo_d + ext_d) per dimension (indices of the full
 * array; ext_d >= 1, lo_d + ext_d <= shape_d; lo and ext are uint64_t[D] on the HOST) of what
 * mgh_prolong writes for the same h, level and d_level, bit for bit -- mgh_prolong's -0.0 exception
 * included, the crop has it too. d_level: the WHOLE dense array of `level`, exactly what mgh_prolong
 * takes; NOT modified. d_out: DENSE in ext (MGH_LD_OUT is not honoured), and not d_level. A NULL
 * pointer, a level outside 0 ... l_target, ext_d == 0 or lo_d + ext_d > shape_d:
 * MGH_ERR_INVALID_ARGUMENT, nothing launched, d_out untouched. level == l_target is a box copy.
 * D = 3 on the fused route: prolongation is local (a node of level l depends on at most two nodes
 * per dimension of level l - 1), so one launch of the window kernel per level above `level` runs
 * over the cells under the window only. The first reads d_level in place, the intermediates live
 * in window-sized buffers of the hierarchy (grown on demand, counted in mgh_device_bytes); no
 * allocation, memset or pass is proportional to the array. Every other shape (D <= 2, thin shapes,
 * D = 4, 5, MGH_FORCE_V1, MGH_FORCE_ND): mgh_prolong into a full-sized array of the hierarchy, and
 * a box copy of the window out of it -- full-sized work, there so that the call has one meaning on
 * every shape. */
int mgh_prolong_window(mgh_hierarchy *h, int level, const void *d_level, const uint64_t *lo, const uint64_t *ext,
                       void *d_out, void *stream);
/* ... into a sub-box of a larger array: d_out points at the element the window's first node goes
 * to, out_stride (uint64_t[D] on the host) are the element strides of that array; the fastest one
 * must be 1. (mgh_decompress_preview_window writes a device-resident output this way.) */
int mgh_prolong_window_strided(mgh_hierarchy *h, int level, const void *d_level, const uint64_t *lo,
                               const uint64_t *ext, void *d_out, const uint64_t *out_stride, void *stream);
/* HOST only, no device work: the nodes mgh_prolong_window's result depends on. For every level
 * l = level ... l_target and every dimension d the closed range of real node indices of level l,
 * out[(l - level) * 2 * D + 2 * d] = first, [... + 1] = last; the ranges of l_target are the window
 * itself. Returns the number of integers written ((l_target - level + 1) * 2 * D <= cap) or a
 * negative status. */
int mgh_debug_prolong_window_ranges(const mgh_hierarchy *h, int level, const uint64_t *lo, const uint64_t *ext,
                                    int64_t *out, uint64_t cap);
/* Developer aid: the launch plan of the window kernel for the step l - 1 -> l
 * (level < l <= l_target) of that window as twelve ints: the six of mgh_debug_prolong_plan, then
 * the first cell and the number of cells per dimension (r, c, f).
 * MGH_ERR_UNSUPPORTED_DIMENSION where mgh_prolong_window runs no kernel of its own. */
int mgh_debug_prolong_window_plan(const mgh_hierarchy *h, int level, const uint64_t *lo, const uint64_t *ext, int l,
                                  int *out12);
/* HOST only: index in the finest grid of every node of `level` along `dim`, ascending
 * (level_shape(level)[dim] entries; returns their number, or a negative status). The rule is the
 * hierarchy's own coarsening, level by level: keep every second node and always the last one. With
 * it a caller builds the coordinates of the coarse grid of a non-uniform array. */
int mgh_level_nodes(const mgh_hierarchy *h, int level, int dim, uint64_t *h_idx_out, uint64_t cap);

/* OutlierRestore (LinearQuantization.hpp:304-350) on its own: d_q[idx[i]] = val[i]; indices
 * outside [0, n) are ignored. */
int mgh_outlier_restore(int64_t *d_q, uint64_t n, const uint64_t *d_outlier_idx,
                        const int64_t *d_outlier_val, uint64_t outlier_count, void *stream);

/* config.reorder == 1 of the reference ("level linearised" quantized output,
 * Quantization/LinearQuantization.hpp:46-146 calc_level_offset, :588-605 slot of a level): the
 * quantized array with the entries of level 0 first, then the coefficients of level 1 in the
 * natural row-major order of the level-1 grid, and so on. A permutation of the reordered N-D
 * array mgh_quantize / mgh_decompose_quantize write; inverse != 0 undoes it. d_in != d_out.
 * d_outlier_idx (optional, forward only): outlier indices are rewritten in place to positions in
 * the linearised array, as the reference records them in this mode (:226-232); their number is
 * outlier_count, or *d_outlier_count (device) capped at outlier_capacity when that is given. */
int mgh_level_linearize(mgh_hierarchy *h, const int64_t *d_in, int64_t *d_out, int inverse,
                        uint64_t *d_outlier_idx, const uint64_t *d_outlier_count, uint64_t outlier_count,
                        uint64_t outlier_capacity, void *stream);

/* Per-kernel timing hook used by bench.py for the roofline line: when enabled,
 * every kernel launched through this handle is bracketed by HIP events on the
 * launch stream; mgh_profile_read() synchronises and returns accumulated
 * milliseconds and launch counts per kernel name since the last reset.
 * (Reference counterpart: DeviceRuntime::TimingAllKernels,
 * src/mgard-x/RuntimeX/DeviceAdapters/DeviceAdapterSerial.cpp:18-19.) */
int mgh_profile_enable(mgh_hierarchy *h, int enable);
/* Restrict the event bracketing to launches of one kernel name (NULL = all), so
 * that a timed region can carry events on its dominant kernel only. */
int mgh_profile_filter(mgh_hierarchy *h, const char *kernel_name_or_null);
/* Writes up to cap entries; returns number of distinct kernels. names[i] points
 * to a static string. */
int mgh_profile_read(mgh_hierarchy *h, const char **names, double *total_ms, uint64_t *launches,
                     int cap, int reset);

/* Test aid (no reference counterpart): while profiling is enabled on a hierarchy, every Thomas
 * solve that goes through the solver's planner (mgard_amd/csrc/ipk_plan.hpp) leaves one record, the
 * first 512 of them since the last reset. A record is MGH_IPK_PLAN_FIELDS values: family (position in
 * IpkKernel: 0 Spec, 1 LdsContigChunked, 2 Dma, 3 Stream, 4 LdsContig, 5 LdsStrided, 6 Thread), axis
 * of the compact box, element size, m[0], m[1], m[2], boxes of the launch, pencil length n, pencils,
 * W, n_glob, KR, P, K, add (0: plain, +1 / -1: added to / subtracted from the coarse nodes), element
 * stride between the boxes. Writes up to cap records to out; returns the number recorded. */
#define MGH_IPK_PLAN_FIELDS 16
int mgh_debug_ipk_plans_read(mgh_hierarchy *h, long long *out, int cap, int reset);

/* Test aid (no reference counterpart): the solves in verified chunks (family Spec) recompute every
 * chunk whose start did not meet the end of the chunk before it, and count those chunks. Waits for
 * the device, then writes to *out the chunks repaired on this hierarchy since it was created or
 * since the last read with reset != 0; 0 if no such solve has run yet. */
int mgh_debug_spec_repairs_read(mgh_hierarchy *h, uint64_t *out, int reset);

/* Test aid (no reference counterpart): while profiling is enabled on a hierarchy, every level that
 * goes through the planner of the fused level passes (mgard_amd/csrc/fused_plan.hpp) leaves one
 * record, the first 512 of them since the last reset. A record is MGH_FUSED_PLAN_FIELDS values: size
 * class, element size, m[0], m[1], m[2] of the coarse box, TC, TF of the main tiles, 1 if the launch
 * has face tiles, tiles, grid.x, march length (coarse planes per r-chunk), r-chunks, 1 if the march
 * was chosen against the residency (0: the class's constant), slices of the first and the second
 * launch (D = 4: even, odd; else 1, 0), workgroups of the two launches, resident workgroups
 * (slots) of the first launch's kernel instance, rounds of resident workgroups (the larger of the
 * two launches'), slots of the second launch's instance. Writes up to cap records to out; returns
 * the number recorded. */
#define MGH_FUSED_PLAN_FIELDS 20
int mgh_debug_fused_plans_read(mgh_hierarchy *h, long long *out, int cap, int reset);

/* ---- Error statistics of two arrays ------------------------------------------------------------
 * What include/mgard-x/Utilities/ErrorCalculator.h computes on the host with one loop per figure
 * (L_inf_norm :22-33, L_2_norm :35-54, L_inf_error :56-72, L_2_error :74-97, MSE :99-107, PSNR
 * :109-121), gathered in ONE pass over both arrays on the device. a = the reference (original)
 * array, b = the other one. Fixed layout, 72 bytes: uint64_t and double fields only.
 *  n            elements compared
 *  nonfinite    positions where a[i] - b[i] is not finite (either value NaN or +-Inf, Inf - Inf, or
 *               a difference that overflows). They are COUNTED HERE AND EXCLUDED FROM EVERY OTHER
 *               FIELD. (The reference lets a NaN poison its sums and ignores it in its maxima.)
 *  max_abs_err  max |a[i] - b[i]|: difference and fabs in the arrays' type, then widened (:57-64)
 *  argmax       flat row-major index in the LOGICAL dense array of the lowest-indexed position that
 *               attains max_abs_err; 0 when no position is finite
 *  sum_sq_err   sum of (double)|a[i] - b[i]| squared, accumulated in double
 *  ref_min, ref_max, ref_abs_max, ref_sum_sq   min a[i], max a[i], max |a[i]|, sum (double)a[i]^2
 *               over the same positions (all 0 when there is none)
 * Derived figures (csrc/compare_plan.hpp, and the C++ / Python mirrors): mse = sum_sq_err /
 * (n - nonfinite), rmse, psnr = 20 log10((ref_max - ref_min) / rmse). */
typedef struct mgh_error_stats {
  uint64_t n;
  uint64_t nonfinite;
  double max_abs_err;
  uint64_t argmax;
  double sum_sq_err;
  double ref_min;
  double ref_max;
  double ref_abs_max;
  double ref_sum_sq;
} mgh_error_stats;

/* D = 1 ... MGH_MAX_DIM, shape[D] on the host. ld_a / ld_b: leading dimensions in mgh_set_ld's
 * convention (D entries, ld[d] >= shape[d] for d >= 1, ld[0] not used), each array its own; NULL =
 * dense. a and b may each be a DEVICE pointer (memory of `device`) or a HOST pointer -- the call
 * finds out itself. Device arrays are read in place, once, by one launch of the reduction kernel
 * (plus a one-workgroup launch that folds the per-workgroup results in a fixed order): no
 * floating-point atomics, and the slabs of the workgroups depend on the number of elements only, so
 * for the same shape and the same position of `a` relative to a 16-byte boundary (which decides the
 * scalar head of a slab) the result is bit-reproducible from call to call and from device to device;
 * at another alignment of `a` only the last bits of the two sums may differ. A host array travels
 * through a device buffer in slabs of at most 64 MB whose results are folded in order (the sums
 * then round differently from the one-launch sums; everything else is exact); with a host array in
 * the call both arrays must be dense (MGH_ERR_INVALID_ARGUMENT otherwise).
 * SYNCHRONOUS: *h_out is filled when the call returns. `stream`: the work is queued there. No
 * hierarchy is needed. The scratch for the per-workgroup results is the call's own for as long as
 * it runs (taken from a list of idle buffers of the device and put back on return), so calls in
 * flight on different streams or threads never share one. The list holds as many buffers (147 KB
 * each) as calls have run at the same time; mgh_release_cache (mgard_hip_compress.h) frees it. Errors (MGH_ERR_INVALID_ARGUMENT, message in mgh_last_error, nothing launched):
 * D outside 1 ... MGH_MAX_DIM, an unknown dtype, a NULL shape / a / b / h_out, ld[d] < shape[d],
 * a device that does not exist. */
int mgh_compare(int D, int dtype, const uint64_t *shape, const void *a, const uint64_t *ld_a,
                const void *b, const uint64_t *ld_b, mgh_error_stats *h_out, int device, void *stream);

/* Measurement aid for the roofline line (no reference counterpart): a PURE stream with the
 * read/write mix of the top-level pass of the hot path -- n elements of `dtype` read once,
 * n int64 written once with streaming stores, two side arrays of n/8 elements written -- and
 * nothing else, timed with HIP events on `stream` over `reps` launches after 2 warm-up
 * launches. *ms_out = average launch time. It tells how fast this device moves the pass's
 * bytes when no arithmetic, halo or tiling is involved (about 4.0 ... 4.9 TB/s, not the 8 TB/s
 * pin rate). d_in: n elements; d_out: n int64; d_side: n/4 elements of `dtype`. */
int mgh_stream_calibrate(int dtype, const void *d_in, int64_t *d_out, void *d_side, uint64_t n,
                         int reps, double *ms_out, void *stream);

/* ---- Missing-value masks (EXTENSION; the reference has nothing here) --------------------------------
 * Arrays with NaN / +-Inf or a fill value (1e20, -9999) must not reach the decomposition: its Thomas
 * solves are global along every dimension. These three streaming passes classify the elements, replace
 * the masked ones by a deterministic fill, and put a value back at the masked positions afterwards.
 * They need no hierarchy: D (1 ... MGH_MAX_DIM), shape[D] on the host, dtype, dense DEVICE arrays on the
 * current device, ASYNCHRONOUS on `stream`. 1 ... 2^32 - 1 elements (MGH_ERR_INVALID_ARGUMENT beyond).
 *
 * The packed mask: ceil(n / 64) uint64_t, bit i % 64 of word i / 64 set when flat element i is masked;
 * the unused high bits of the last word are zero.
 *
 * mgh_mask_scan: flags = MGH_MASK_NONFINITE (NaN, +-Inf) | MGH_MASK_VALUE (x == (T)fill_value); 0 and a
 * NaN fill_value with MGH_MASK_VALUE are MGH_ERR_INVALID_ARGUMENT. Writes `words` and the device
 * mgh_mask_stats: n, n_masked and the extremes of the VALID elements (vmin = vmax = 0 when there is
 * none; -0.0 orders below +0.0). Count, minimum and maximum do not depend on the order of the
 * reduction: the result is deterministic.
 *
 * mgh_mask_fill: out (may be data) = data with every masked element replaced. THE RULE IS PART OF THE
 * INTERFACE -- it can be restated in NumPy to the bit: rows run along the last (fastest) dimension, of
 * length nf; every row is cut into segments [k 1024, min((k + 1) 1024, nf)), restarting at every row; a
 * masked element takes the value of the nearest valid element with a SMALLER index in its segment, if
 * there is none of the nearest one with a LARGER index in its segment, and (T)c if the segment has no
 * valid element. Valid elements are copied bit for bit; only copies and the one constant occur.
 *
 * mgh_mask_restore: data[i] = (T)value (which may be NaN) at every masked i; the rest is untouched. */
#define MGH_MASK_NONFINITE 1
#define MGH_MASK_VALUE 2
typedef struct mgh_mask_stats {
  uint64_t n, n_masked;
  double vmin, vmax;
} mgh_mask_stats;
int mgh_mask_scan(int D, int dtype, const uint64_t *shape, const void *data, int flags, double fill_value,
                  uint64_t *words, mgh_mask_stats *stats, void *stream);
int mgh_mask_fill(int D, int dtype, const uint64_t *shape, const void *data, const uint64_t *words, double c,
                  void *out, void *stream);
int mgh_mask_restore(int D, int dtype, const uint64_t *shape, const uint64_t *words, double value, void *data,
                     void *stream);

/* ---- Pointwise relative error bound (EXTENSION; the reference has nothing here) ----------------------
 * The result types of the three streaming passes behind mgh_compress_pwrel / mgh_decompress_pwrel /
 * mgh_verify_pwrel (mgard_hip_compress.h; classes, tolerance and trailer: csrc/pwrel_plan.hpp). An element x of
 * type T is, against floor_eff = max(abs_floor, smallest normal of T):
 *   nonfinite (NaN, +-Inf): mask bit 1, flag bit 1, decodes to a quiet NaN;
 *   zeroed (|x| < floor_eff: +-0, denormals, small values): mask bit 1, flag bit 0, decodes to +0.0;
 *   valid (the rest): mask bit 0, flag bit = sign of x, decodes to +-exp2(y').
 * Both bitmaps have the layout of the packed mask above. The passes themselves -- forward (one read of x:
 * y = (T)log2((double)|x|), both bitmaps by wave ballots, mgh_pwrel_stats), inverse (in place over the decoded y',
 * the magnitude clamped to [smallest normal, largest finite] of T) and compare (mgh_pwrel_compare of an original
 * against a reconstruction) -- are exported with a trailing underscore and declared in no public header yet, like
 * mgh_mask_sample_: a function declared here with a stream parameter must have its row in the stream-order
 * table of the test suite, which a later change adds together with the declarations.
 * mgh_pwrel_stats: ymin / ymax are the extremes of y over the VALID elements (0, 0 when there is none);
 * n_nonfinite of the n_masked are non-finite; n_flag counts the set flag bits (non-finite and negative valid).
 * mgh_pwrel_compare: max_rel_err = max |x' - x| / |x| in double over the valid positions whose x' is finite, at
 * flat index argmax (the lowest on a tie; 0, 0 when there is none); max_zeroed_abs: the largest |x| among zeroed
 * positions; n_class_mismatch: a zeroed position that is not +0.0 to the bit, a non-finite position that is not
 * NaN, or a valid position that is not finite and non-zero; n_sign_mismatch: a valid position, finite and
 * non-zero, with the other sign. */
typedef struct mgh_pwrel_stats {
  uint64_t n, n_masked, n_nonfinite, n_flag;
  double ymin, ymax;
} mgh_pwrel_stats;
typedef struct mgh_pwrel_compare {
  uint64_t n, n_valid, n_zeroed, n_nonfinite;
  double max_rel_err;
  uint64_t argmax;
  double max_zeroed_abs;
  uint64_t n_class_mismatch, n_sign_mismatch;
} mgh_pwrel_compare;

#ifdef __cplusplus
}
#endif
#endif /* MGARD_HIP_H */
