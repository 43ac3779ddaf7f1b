/* mgard_hip_level_layers.h -- the low-level calls of the precision layers in LEVEL ORDER (DESIGN.md
 * section 8), on top of mgard_hip.h (which this header includes; mgard_hip.h does not include it).
 *
 * They stand in a file of their own because tests/test_stream_cases_cpu.py ties every stream-taking
 * declaration of mgard_hip.h to a row of the stream-order table in tests/test_gpu_stream_order.py; these
 * three have their stream-order cases in tests/test_gpu_stream_level_layers.py (a table of the same form,
 * which tests/test_level_layers_abi_cpu.py ties to this header the same way). When that table is next
 * revised the rows move there and the declarations into mgard_hip.h. */
#ifndef MGARD_HIP_LEVEL_LAYERS_H
#define MGARD_HIP_LEVEL_LAYERS_H

#include "mgard_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Precision layers in LEVEL ORDER: the two calls above on the level-linearised
 * layout of a reorder = 1 record, so that a layer can be read up to a level from the head of its record.
 * Dense arrays only; arrays of 2^32 elements and more are refused. ASYNCHRONOUS behind the upload of the
 * quantizer tables. No reference counterparts.
 *
 * mgh_quantize_residual_linear (the writer's quantizing step): d_linear_out [total int64] and the outlier
 * pairs (as a set; the indices are LINEARISED positions) are what mgh_quantize(prep_huffman = 1) followed by
 * mgh_level_linearize(forward, with the index list) give; the call zeroes the counter as mgh_quantize does.
 * d_residual_out is mgh_quantize_symbols_residual's residual, bit for bit, in ARRAY order (in place over a
 * dense d_coeff is allowed). The integers pass through a full-sized int64 buffer of the hierarchy (counted
 * in mgh_device_bytes). Refusals: those of mgh_quantize_symbols_residual.
 *
 * mgh_dequantize_add_linear (the reader's kernel): d_linear_window holds the integers [first, first + count)
 * of the level-linearised array, d_acc_linear is the WHOLE accumulator (total elements of the hierarchy's
 * type) in level-linearised order. Outlier indices are linearised positions of the whole array: those
 * inside the window are written into d_linear_window first (it is modified), all others are skipped. For
 * every position p of the window: acc[p] = (store ? nothing : acc[p]) + mgh_dequantize's value of that
 * integer at the node p stands for -- inside the window bit for bit the forward linearisation of what
 * mgh_dequantize_add leaves for the inverse-linearised integers. Nothing outside the window is read or
 * written. count == 0 or a window that leaves the array: MGH_ERR_INVALID_ARGUMENT. */
int mgh_quantize_residual_linear(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, double s,
                                 double norm, uint64_t dict_size, int64_t *d_linear_out, uint64_t *d_outlier_count,
                                 uint64_t *d_outlier_idx, int64_t *d_outlier_val, uint64_t outlier_capacity,
                                 void *d_residual_out, void *stream);
int mgh_dequantize_add_linear(mgh_hierarchy *h, int64_t *d_linear_window, uint64_t first, uint64_t count,
                              int error_bound_type, double tol, double s, double norm, uint64_t dict_size,
                              int prep_huffman, const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                              uint64_t outlier_count, int store, void *d_acc_linear, void *stream);

/* mgh_recompose_to_level from the HEAD of a level-linearised COEFFICIENT array (the accumulator of
 * mgh_dequantize_add_linear): only its first N_level elements are read, as the compact corner box of
 * `level` (a buffer of the hierarchy, counted in mgh_device_bytes). d_out is dense in level_shape(level),
 * bit-identical to mgh_recompose_to_level on the same coefficients in array order, and at
 * level == l_target to mgh_recompose. d_acc_linear is not modified; d_out must not be d_acc_linear. Below
 * l_target no work scales with the full array. Arrays of 2^32 elements and more are refused. */
int mgh_recompose_linear_to_level(mgh_hierarchy *h, const void *d_acc_linear, int level, void *d_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MGARD_HIP_LEVEL_LAYERS_H */
