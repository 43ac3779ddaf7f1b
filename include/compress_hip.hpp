// compress_hip.hpp -- C++ mirror of the reference's HIGH-LEVEL API (include/compress_x.hpp:31-178)
// on top of the C ABI of mgard_hip_compress.h. Header only. Same names, argument order,
// ownership rules and status codes as mgard_x::compress / decompress, so that a caller switches
// by changing the namespace:
//
//   mgard_hip::Config config;                       // defaults of Config.cpp:14-43
//   config.lossless = mgard_hip::lossless_type::Huffman_Zstd;
//   void *compressed = nullptr; size_t compressed_size = 0;
//   mgard_hip::compress(3, mgard_hip::data_type::Float, {512, 512, 512}, 1e-3,
//                       std::numeric_limits<double>::infinity(), mgard_hip::error_bound_type::REL,
//                       data, compressed, compressed_size, config, false);
//   void *out = nullptr;
//   mgard_hip::decompress(compressed, compressed_size, out, config, false);
//
// Buffers may be host or device memory; outputs that are not pre-allocated are malloc'ed (host
// input) or hipMalloc'ed (device input) by the library and belong to the caller
// (CompressionHighLevel.hpp:147-162).
#ifndef COMPRESS_HIP_HPP
#define COMPRESS_HIP_HPP

#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "mgard_hip.hpp"
#include "mgard_hip_compress.h"
#include "mgard_hip_errors.hpp"

namespace mgard_hip {

using Byte = unsigned char;                                                 // DataTypes.h:126
enum class domain_decomposition_type : uint8_t { MaxDim, Block, Variable };  // Types.h:50
enum class lossless_type : uint8_t { Huffman, Huffman_LZ4, Huffman_Zstd, CPU_Lossless };

// mgard_x::Config (Config/Config.h:10-42): the fields the high-level path reads
struct HighLevelConfig : Config {
  domain_decomposition_type domain_decomposition = domain_decomposition_type::MaxDim;
  int domain_decomposition_dim = 0;
  std::vector<SIZE> domain_decomposition_sizes;
  SIZE block_size = 256;
  SIZE huff_block_size = 1024 * 20;
  lossless_type lossless = lossless_type::Huffman;
  int zstd_compress_level = 3;
  SIZE max_memory_footprint = std::numeric_limits<SIZE>::max();
  bool auto_pin_host_buffers = false;  // (reference: true; see mgh_config_default in highlevel.hip)
  int reorder = 0;                     // Config::reorder: 1 = level-linearised records (what ProgressiveReader reads)
};

namespace detail {
inline mgh_config to_c(const HighLevelConfig &c) {
  mgh_config m;
  mgh_config_default(&m);
  m.dev_id = c.dev_id;
  m.domain_decomposition = (int)c.domain_decomposition;
  m.domain_decomposition_dim = c.domain_decomposition_dim;
  m.domain_decomposition_sizes = c.domain_decomposition_sizes.empty() ? nullptr : c.domain_decomposition_sizes.data();
  m.num_domain_decomposition_sizes = c.domain_decomposition_sizes.size();
  m.block_size = c.block_size;
  m.estimate_outlier_ratio = c.estimate_outlier_ratio;
  m.huff_dict_size = c.huff_dict_size;
  m.huff_block_size = c.huff_block_size;
  m.lossless = (int)c.lossless;
  m.zstd_compress_level = c.zstd_compress_level;
  m.normalize_coordinates = c.normalize_coordinates ? 1 : 0;
  m.max_larget_level = c.max_larget_level;
  m.max_memory_footprint = c.max_memory_footprint;
  m.auto_pin_host_buffers = c.auto_pin_host_buffers ? 1 : 0;
  m.reorder = c.reorder;
  return m;
}
inline compress_status_type status(int rc) {
  if (rc == MGH_ERR_OUTPUT_TOO_LARGE) return compress_status_type::OutputTooLargeFailure;
  return to_status(rc);
}
} // namespace detail

// compress (compress_x.hpp:56-76): non-uniform grid, explicit config
inline compress_status_type compress(DIM D, data_type dtype, std::vector<SIZE> shape, double tol, double s,
                                     error_bound_type mode, const void *original_data,
                                     void *&compressed_data, size_t &compressed_size,
                                     std::vector<const Byte *> coords, HighLevelConfig config,
                                     bool output_pre_allocated) {
  if (shape.size() != D) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress(D, (int)dtype, shape.data(), tol, s, (int)mode, original_data,
                                     &compressed_data, &compressed_size, cp.empty() ? nullptr : cp.data(),
                                     &c, output_pre_allocated ? 1 : 0));
}
// (compress_x.hpp:44-54)
inline compress_status_type compress(DIM D, data_type dtype, std::vector<SIZE> shape, double tol, double s,
                                     error_bound_type mode, const void *original_data,
                                     void *&compressed_data, size_t &compressed_size,
                                     HighLevelConfig config, bool output_pre_allocated) {
  return compress(D, dtype, shape, tol, s, mode, original_data, compressed_data, compressed_size,
                  std::vector<const Byte *>(), config, output_pre_allocated);
}
// (compress_x.hpp:31-42)
inline compress_status_type compress(DIM D, data_type dtype, std::vector<SIZE> shape, double tol, double s,
                                     error_bound_type mode, const void *original_data,
                                     void *&compressed_data, size_t &compressed_size,
                                     bool output_pre_allocated) {
  return compress(D, dtype, shape, tol, s, mode, original_data, compressed_data, compressed_size,
                  HighLevelConfig(), output_pre_allocated);
}
// (compress_x.hpp:78-100)
inline compress_status_type compress(DIM D, data_type dtype, std::vector<SIZE> shape, double tol, double s,
                                     error_bound_type mode, const void *original_data,
                                     void *&compressed_data, size_t &compressed_size,
                                     std::vector<const Byte *> coords, bool output_pre_allocated) {
  return compress(D, dtype, shape, tol, s, mode, original_data, compressed_data, compressed_size, coords,
                  HighLevelConfig(), output_pre_allocated);
}

// decompress (compress_x.hpp:109-154)
inline compress_status_type decompress(const void *compressed_data, size_t compressed_size,
                                       void *&decompressed_data, HighLevelConfig config,
                                       bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress(compressed_data, compressed_size, &decompressed_data, &c,
                                       output_pre_allocated ? 1 : 0));
}
inline compress_status_type decompress(const void *compressed_data, size_t compressed_size,
                                       void *&decompressed_data, bool output_pre_allocated) {
  return decompress(compressed_data, compressed_size, decompressed_data, HighLevelConfig(),
                    output_pre_allocated);
}
// EXTENSION (the reference's decompress has no level argument): the array at `level` of the
// hierarchy (0 = coarsest), dense in the shape infer_level_shape gives; containers with one
// subdomain only (mgh_decompress_level).
inline compress_status_type decompress_level(const void *compressed_data, size_t compressed_size, int level,
                                             void *&decompressed_data, HighLevelConfig config,
                                             bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_level(compressed_data, compressed_size, level, &decompressed_data, &c,
                                             output_pre_allocated ? 1 : 0));
}
// shape of `level` and l_target of the container's hierarchy; level < 0: only l_target (shape left
// empty). The status tells a failure from that query.
inline compress_status_type infer_level_shape(const void *compressed_data, size_t compressed_size, int level,
                                              HighLevelConfig config, std::vector<SIZE> &shape, int &l_target) {
  const mgh_config c = detail::to_c(config);
  int D = 0, lt = 0;
  uint64_t shp[MGH_MAX_DIM];
  shape.clear();
  const int rc = mgh_infer_level_shape(compressed_data, compressed_size, &c, level, &D, shp, &lt);
  if (rc != MGH_SUCCESS) return detail::status(rc);
  l_target = lt;
  if (level >= 0) shape.assign(shp, shp + D);
  return compress_status_type::Success;
}
// EXTENSION: reduced resolution of any container, domain-decomposed ones included. `halvings` counts
// coarsenings of the grid (n -> n/2 + 1), the same in every subdomain; the result is the subdomains'
// level arrays stitched into one dense array of the shape infer_coarsened_shape gives
// (mgh_decompress_coarsened).
inline compress_status_type decompress_coarsened(const void *compressed_data, size_t compressed_size, int halvings,
                                                 void *&decompressed_data, HighLevelConfig config,
                                                 bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_coarsened(compressed_data, compressed_size, halvings, &decompressed_data, &c,
                                                 output_pre_allocated ? 1 : 0));
}
// EXTENSION: full-grid preview (mgh_decompress_preview). The container after `halvings` coarsenings,
// every subdomain prolonged back to its own grid: an array of the container's shape and type, placed
// like decompress places it. halvings = 0 is decompress.
inline compress_status_type decompress_preview(const void *compressed_data, size_t compressed_size, int halvings,
                                               void *&decompressed_data, HighLevelConfig config,
                                               bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_preview(compressed_data, compressed_size, halvings, &decompressed_data, &c,
                                               output_pre_allocated ? 1 : 0));
}
// EXTENSION: mgh_verify. The error statistics of `original_data` (host or device memory) against what
// decompress -- halvings = 0 -- or decompress_preview would write, subdomain by subdomain on the device,
// without that array being made; result.within tells whether the container keeps its bound.
inline compress_status_type verify(const void *compressed_data, size_t compressed_size, const void *original_data,
                                   size_t original_bytes, data_type dtype, int halvings, HighLevelConfig config,
                                   mgh_verify_result &result) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_verify(compressed_data, compressed_size, original_data, original_bytes, (int)dtype, halvings,
                                   &c, &result));
}
// EXTENSION: mgh_estimate_sizes. What compress(tol) would write for every tolerance of `tols` (1..64),
// from one decomposition: estimates[k].bytes_min <= size <= bytes_max. Containers of one subdomain,
// lossless_type::Huffman only (Failure otherwise; mgh_last_error() says which).
inline compress_status_type estimate_sizes(DIM D, data_type dtype, std::vector<SIZE> shape,
                                           const std::vector<double> &tols, double s, error_bound_type mode,
                                           const void *original_data, std::vector<const Byte *> coords,
                                           HighLevelConfig config, std::vector<mgh_size_estimate> &estimates) {
  if (shape.size() != D) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  estimates.assign(tols.size(), mgh_size_estimate{});
  return detail::status(mgh_estimate_sizes(D, (int)dtype, shape.data(), (int)tols.size(), tols.data(), s, (int)mode,
                                           original_data, cp.empty() ? nullptr : cp.data(), &c, estimates.data()));
}
// EXTENSION: mgh_compress_budget. The most accurate container of at most max_bytes with a tolerance in
// [tol_min, tol_max] (`rounds` in 1..8 rounds of the search): the container compress(tol_used) writes.
// OutputTooLargeFailure when not even tol_max fits (nothing allocated).
inline compress_status_type compress_budget(DIM D, data_type dtype, std::vector<SIZE> shape, size_t max_bytes,
                                            double tol_min, double tol_max, int rounds, double s, error_bound_type mode,
                                            const void *original_data, void *&compressed_data, size_t &compressed_size,
                                            std::vector<const Byte *> coords, HighLevelConfig config,
                                            bool output_pre_allocated, double &tol_used,
                                            mgh_size_estimate *estimate_used = nullptr) {
  if (shape.size() != D) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress_budget(D, (int)dtype, shape.data(), max_bytes, tol_min, tol_max, rounds, s, (int)mode,
                                            original_data, &compressed_data, &compressed_size,
                                            cp.empty() ? nullptr : cp.data(), &c, output_pre_allocated ? 1 : 0, &tol_used,
                                            estimate_used));
}
// EXTENSION: mgh_compress_ladder. compressed_data[k] / compressed_size[k]: the container compress(tols[k])
// writes (up to the order of its outlier list), for every tolerance of `tols` (1..64) in order, from ONE
// decomposition. Containers of one subdomain (Failure otherwise; mgh_last_error() says so). Without
// output_pre_allocated both vectors are sized here and every container is the caller's to free as
// compress's is; with it, they carry the buffers and their capacities in. When tolerance k fails the
// status is that write's, the containers before k stay valid and the pointers from k on are null where
// the call allocates them.
inline compress_status_type compress_ladder(DIM D, data_type dtype, std::vector<SIZE> shape,
                                            const std::vector<double> &tols, double s, error_bound_type mode,
                                            const void *original_data, std::vector<void *> &compressed_data,
                                            std::vector<size_t> &compressed_size, std::vector<const Byte *> coords,
                                            HighLevelConfig config, bool output_pre_allocated) {
  if (shape.size() != D) return compress_status_type::Failure;
  if (output_pre_allocated && (compressed_data.size() != tols.size() || compressed_size.size() != tols.size()))
    return compress_status_type::Failure;
  if (!output_pre_allocated) {
    compressed_data.assign(tols.size(), nullptr);
    compressed_size.assign(tols.size(), 0);
  }
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress_ladder(D, (int)dtype, shape.data(), (int)tols.size(), tols.data(), s, (int)mode,
                                            original_data, compressed_data.data(), compressed_size.data(),
                                            cp.empty() ? nullptr : cp.data(), &c, output_pre_allocated ? 1 : 0));
}
// EXTENSION: mgh_compress_layers. compressed_data[k]: the layer of tols[k] (strictly decreasing, 1..64) --
// what the layers before it left of the coefficients, quantized at tols[k]; layer 0 is compress(tols[0])'s
// container. Vectors, allocation and the failure at layer k as in compress_ladder. Containers of one
// subdomain, reorder = 0 (Failure otherwise; mgh_last_error() says so). The order of the layers is the
// caller's to keep: the containers carry no index.
inline compress_status_type compress_layers(DIM D, data_type dtype, std::vector<SIZE> shape,
                                            const std::vector<double> &tols, double s, error_bound_type mode,
                                            const void *original_data, std::vector<void *> &compressed_data,
                                            std::vector<size_t> &compressed_size, std::vector<const Byte *> coords,
                                            HighLevelConfig config, bool output_pre_allocated) {
  if (shape.size() != D) return compress_status_type::Failure;
  if (output_pre_allocated && (compressed_data.size() != tols.size() || compressed_size.size() != tols.size()))
    return compress_status_type::Failure;
  if (!output_pre_allocated) {
    compressed_data.assign(tols.size(), nullptr);
    compressed_size.assign(tols.size(), 0);
  }
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress_layers(D, (int)dtype, shape.data(), (int)tols.size(), tols.data(), s, (int)mode,
                                            original_data, compressed_data.data(), compressed_size.data(),
                                            cp.empty() ? nullptr : cp.data(), &c, output_pre_allocated ? 1 : 0));
}
// ... and its one-shot reader (mgh_decompress_layers): the array after layers 0 .. size() - 1, in order.
inline compress_status_type decompress_layers(const std::vector<const void *> &compressed_data,
                                              const std::vector<size_t> &compressed_size, void *&decompressed_data,
                                              HighLevelConfig config, bool output_pre_allocated) {
  if (compressed_data.size() != compressed_size.size()) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_layers((int)compressed_data.size(), compressed_data.data(), compressed_size.data(),
                                              &c, &decompressed_data, output_pre_allocated ? 1 : 0));
}
// EXTENSION: mgh_compress_level_layers: compress_layers with level-linearised records (reorder = 1 whatever
// config.reorder says), so that a reader takes level L of layer k from the head of that layer's record
// (LevelLayersReader, decompress_level_layers). Layer 0 is compress(tols[0], reorder = 1)'s container.
inline compress_status_type compress_level_layers(DIM D, data_type dtype, std::vector<SIZE> shape,
                                                  const std::vector<double> &tols, double s, error_bound_type mode,
                                                  const void *original_data, std::vector<void *> &compressed_data,
                                                  std::vector<size_t> &compressed_size, std::vector<const Byte *> coords,
                                                  HighLevelConfig config, bool output_pre_allocated) {
  if (shape.size() != D) return compress_status_type::Failure;
  if (output_pre_allocated && (compressed_data.size() != tols.size() || compressed_size.size() != tols.size()))
    return compress_status_type::Failure;
  if (!output_pre_allocated) {
    compressed_data.assign(tols.size(), nullptr);
    compressed_size.assign(tols.size(), 0);
  }
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress_level_layers(D, (int)dtype, shape.data(), (int)tols.size(), tols.data(), s, (int)mode,
                                                  original_data, compressed_data.data(), compressed_size.data(),
                                                  cp.empty() ? nullptr : cp.data(), &c, output_pre_allocated ? 1 : 0));
}
// ... and its one-shot reader (mgh_decompress_level_layers): level `level` of the array after layers
// 0 .. size() - 1, every layer read up to that level. The output is dense in the level's shape
// (mgh_infer_level_shape).
inline compress_status_type decompress_level_layers(const std::vector<const void *> &compressed_data,
                                                    const std::vector<size_t> &compressed_size, int level,
                                                    void *&decompressed_data, HighLevelConfig config,
                                                    bool output_pre_allocated) {
  if (compressed_data.size() != compressed_size.size()) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_level_layers((int)compressed_data.size(), compressed_data.data(),
                                                    compressed_size.data(), level, &c, &decompressed_data,
                                                    output_pre_allocated ? 1 : 0));
}
// EXTENSION: mgh_compress_masked. compress of an array whose NaN / +-Inf (spec.flags & MGH_MASK_NONFINITE) and / or
// elements equal to spec.fill_value (MGH_MASK_VALUE) do not count: [container of the filled array][mask record][footer].
// The first masked_info().container_size bytes open in every reader; the bound holds at every valid position.
inline compress_status_type compress_masked(DIM D, data_type dtype, std::vector<SIZE> shape, double tol, double s,
                                            error_bound_type mode, const void *original_data, const mgh_mask_spec &spec,
                                            void *&compressed_data, size_t &compressed_size,
                                            std::vector<const Byte *> coords, HighLevelConfig config,
                                            bool output_pre_allocated) {
  if (shape.size() != D) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress_masked(D, (int)dtype, shape.data(), tol, s, (int)mode, original_data, &spec,
                                            &compressed_data, &compressed_size, cp.empty() ? nullptr : cp.data(), &c,
                                            output_pre_allocated ? 1 : 0));
}
// ... its reader (mgh_decompress_masked): spec.restore_value at every masked position. A plain container is a Failure.
inline compress_status_type decompress_masked(const void *compressed_data, size_t compressed_size,
                                              void *&decompressed_data, HighLevelConfig config,
                                              bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_masked(compressed_data, compressed_size, &c, &decompressed_data,
                                              output_pre_allocated ? 1 : 0));
}
// ... and what the buffer is (mgh_masked_info): masked = false for a plain container (info untouched); a footer
// that fails a check is a Failure.
inline compress_status_type masked_info(const void *compressed_data, size_t compressed_size, bool &masked,
                                        struct mgh_masked_info &info) {
  const int rc = mgh_masked_info(compressed_data, compressed_size, &info);
  masked = rc == 1;
  return rc < 0 ? detail::status(rc) : compress_status_type::Success;
}
// EXTENSION: masked buffers in the reduced-resolution and preview readers (mgh_decompress_masked_level /
// _coarsened / _preview / _preview_window). A node is masked when the element of the full array it stands on is
// masked (sampling); masked positions hold spec.restore_value, every other position what the reader of the same
// name without `masked_` writes for the container part. A plain container is a Failure.
inline compress_status_type decompress_masked_level(const void *compressed_data, size_t compressed_size, int level,
                                                    void *&decompressed_data, HighLevelConfig config,
                                                    bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_masked_level(compressed_data, compressed_size, level, &decompressed_data, &c,
                                                    output_pre_allocated ? 1 : 0));
}
inline compress_status_type decompress_masked_coarsened(const void *compressed_data, size_t compressed_size, int halvings,
                                                        void *&decompressed_data, HighLevelConfig config,
                                                        bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_masked_coarsened(compressed_data, compressed_size, halvings, &decompressed_data, &c,
                                                        output_pre_allocated ? 1 : 0));
}
inline compress_status_type decompress_masked_preview(const void *compressed_data, size_t compressed_size, int halvings,
                                                      void *&decompressed_data, HighLevelConfig config,
                                                      bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_masked_preview(compressed_data, compressed_size, halvings, &decompressed_data, &c,
                                                      output_pre_allocated ? 1 : 0));
}
inline compress_status_type decompress_masked_preview_window(const void *compressed_data, size_t compressed_size,
                                                             int halvings, const std::vector<SIZE> &lo,
                                                             const std::vector<SIZE> &ext, void *&decompressed_data,
                                                             HighLevelConfig config, bool output_pre_allocated) {
  if (lo.size() != ext.size()) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_masked_preview_window(compressed_data, compressed_size, halvings, lo.data(),
                                                             ext.data(), &decompressed_data, &c,
                                                             output_pre_allocated ? 1 : 0));
}
// ... the sampled mask alone, one byte per element of the level array, the coarsened array or the window
inline compress_status_type decompress_mask_level(const void *compressed_data, size_t compressed_size, int level,
                                                  HighLevelConfig config, uint8_t *mask) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_mask_level(compressed_data, compressed_size, level, &c, mask));
}
inline compress_status_type decompress_mask_coarsened(const void *compressed_data, size_t compressed_size, int halvings,
                                                      HighLevelConfig config, uint8_t *mask) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_mask_coarsened(compressed_data, compressed_size, halvings, &c, mask));
}
inline compress_status_type decompress_mask_window(const void *compressed_data, size_t compressed_size,
                                                   const std::vector<SIZE> &lo, const std::vector<SIZE> &ext,
                                                   HighLevelConfig config, uint8_t *mask) {
  if (lo.size() != ext.size()) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_mask_window(compressed_data, compressed_size, lo.data(), ext.data(), &c, mask));
}
// ... and mgh_verify_masked: verify against the user's own array, marks included; masked positions take part in
// nothing (result.stats.n counts the valid ones, n_masked the others).
inline compress_status_type verify_masked(const void *compressed_data, size_t compressed_size, const void *original_data,
                                          size_t original_bytes, data_type dtype, int halvings, HighLevelConfig config,
                                          mgh_verify_result &result, uint64_t &n_masked) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_verify_masked(compressed_data, compressed_size, original_data, original_bytes, (int)dtype,
                                          halvings, &c, &result, &n_masked));
}
// EXTENSION: mgh_compress_pwrel. |x' - x| <= eps |x| at every element: the masked writer around y = log2|x| under an
// ABS bound derived from eps, with the signs in a second bitmap: [masked buffer of y][flag record][footer]. +-0,
// denormals and |x| < abs_floor decode to +0.0, NaN / +-Inf to NaN. An eps the data type cannot carry is a Failure.
inline compress_status_type compress_pwrel(DIM D, data_type dtype, std::vector<SIZE> shape, double eps, double abs_floor,
                                           const void *original_data, void *&compressed_data, size_t &compressed_size,
                                           std::vector<const Byte *> coords, HighLevelConfig config,
                                           bool output_pre_allocated) {
  if (shape.size() != D) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress_pwrel(D, (int)dtype, shape.data(), eps, abs_floor, original_data, &compressed_data,
                                           &compressed_size, cp.empty() ? nullptr : cp.data(), &c,
                                           output_pre_allocated ? 1 : 0));
}
// ... its reader (mgh_decompress_pwrel). A plain container or a masked buffer is a Failure.
inline compress_status_type decompress_pwrel(const void *compressed_data, size_t compressed_size, void *&decompressed_data,
                                             HighLevelConfig config, bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_pwrel(compressed_data, compressed_size, &c, &decompressed_data,
                                             output_pre_allocated ? 1 : 0));
}
// ... and its readers at reduced resolution and in previews (mgh_decompress_pwrel_level / _coarsened / _preview /
// _preview_window). A node takes its class and sign from the element of the full array it stands on (sampling); a
// valid node is +-exp2 of what the reader of the same name without `pwrel_` writes for the container part. Such an
// output carries no error bound. A plain container or a masked buffer is a Failure.
inline compress_status_type decompress_pwrel_level(const void *compressed_data, size_t compressed_size, int level,
                                                   void *&decompressed_data, HighLevelConfig config,
                                                   bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_pwrel_level(compressed_data, compressed_size, level, &decompressed_data, &c,
                                                   output_pre_allocated ? 1 : 0));
}
inline compress_status_type decompress_pwrel_coarsened(const void *compressed_data, size_t compressed_size, int halvings,
                                                       void *&decompressed_data, HighLevelConfig config,
                                                       bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_pwrel_coarsened(compressed_data, compressed_size, halvings, &decompressed_data, &c,
                                                       output_pre_allocated ? 1 : 0));
}
inline compress_status_type decompress_pwrel_preview(const void *compressed_data, size_t compressed_size, int halvings,
                                                     void *&decompressed_data, HighLevelConfig config,
                                                     bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_pwrel_preview(compressed_data, compressed_size, halvings, &decompressed_data, &c,
                                                     output_pre_allocated ? 1 : 0));
}
inline compress_status_type decompress_pwrel_preview_window(const void *compressed_data, size_t compressed_size,
                                                            int halvings, const std::vector<SIZE> &lo,
                                                            const std::vector<SIZE> &ext, void *&decompressed_data,
                                                            HighLevelConfig config, bool output_pre_allocated) {
  if (lo.size() != ext.size()) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_pwrel_preview_window(compressed_data, compressed_size, halvings, lo.data(),
                                                            ext.data(), &decompressed_data, &c,
                                                            output_pre_allocated ? 1 : 0));
}
// ... what the buffer is (mgh_pwrel_info): pwrel = false for any other buffer (info untouched); a footer that fails
// a check is a Failure.
inline compress_status_type pwrel_info(const void *compressed_data, size_t compressed_size, bool &pwrel,
                                       struct mgh_pwrel_info &info) {
  const int rc = mgh_pwrel_info(compressed_data, compressed_size, &info);
  pwrel = rc == 1;
  return rc < 0 ? detail::status(rc) : compress_status_type::Success;
}
// ... and mgh_verify_pwrel: the decoded array against the user's own; within = the bound holds at every valid
// element, every class and sign came back, and nothing at or above the floor was zeroed.
inline compress_status_type verify_pwrel(const void *compressed_data, size_t compressed_size, const void *original_data,
                                         size_t original_bytes, data_type dtype, HighLevelConfig config,
                                         mgh_pwrel_compare &result, bool &within) {
  const mgh_config c = detail::to_c(config);
  int w = 0;
  const int rc = mgh_verify_pwrel(compressed_data, compressed_size, original_data, original_bytes, (int)dtype, &c, &result, &w);
  within = w == 1;
  return detail::status(rc);
}
// EXTENSION: mgh_compress_roi. The array within tol everywhere and within boxes[i].tol at every element of box i (up
// to 16 disjoint boxes, every extent at least 3, s infinite): [container of compress(tol)][one residual record per
// box][box table][footer]. The first bytes open in every plain reader as the unrefined base. A tol_i the data type
// cannot carry is a Failure.
inline compress_status_type compress_roi(DIM D, data_type dtype, std::vector<SIZE> shape, double tol, double s,
                                         error_bound_type mode, const void *original_data,
                                         const std::vector<mgh_roi_box> &boxes, void *&compressed_data,
                                         size_t &compressed_size, std::vector<const Byte *> coords, HighLevelConfig config,
                                         bool output_pre_allocated) {
  if (shape.size() != D) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress_roi(D, (int)dtype, shape.data(), tol, s, (int)mode, original_data, (int)boxes.size(),
                                         boxes.data(), &compressed_data, &compressed_size, cp.empty() ? nullptr : cp.data(),
                                         &c, output_pre_allocated ? 1 : 0));
}
// ... its reader (mgh_decompress_roi). Any buffer without the box footer is a Failure.
inline compress_status_type decompress_roi(const void *compressed_data, size_t compressed_size, void *&decompressed_data,
                                           HighLevelConfig config, bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_roi(compressed_data, compressed_size, &decompressed_data, &c,
                                           output_pre_allocated ? 1 : 0));
}
// ... what the buffer is (mgh_roi_info): roi = false for any other buffer (info untouched); a footer or table that
// fails a check is a Failure.
inline compress_status_type roi_info(const void *compressed_data, size_t compressed_size, bool &roi,
                                     struct mgh_roi_info &info) {
  const int rc = mgh_roi_info(compressed_data, compressed_size, &info);
  roi = rc == 1;
  return rc < 0 ? detail::status(rc) : compress_status_type::Success;
}
// ... and mgh_verify_roi: the decoded array against the user's own, over the whole array against the base bound and
// over every box against that box's (per_box is resized to the number of boxes).
inline compress_status_type verify_roi(const void *compressed_data, size_t compressed_size, const void *original_data,
                                       size_t original_bytes, data_type dtype, HighLevelConfig config,
                                       mgh_verify_result &whole, std::vector<mgh_verify_result> &per_box) {
  struct mgh_roi_info info;
  const int rc = mgh_roi_info(compressed_data, compressed_size, &info);
  if (rc < 0) return detail::status(rc);
  per_box.assign(rc == 1 ? (size_t)info.nbox : 1, mgh_verify_result{});
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_verify_roi(compressed_data, compressed_size, original_data, original_bytes, (int)dtype, &c,
                                       &whole, per_box.data()));
}
// EXTENSION: mgh_achieved_errors. What verify(compress(tol)) would report for every tolerance of `tols`
// (1..64), from one decomposition and without writing a container. Containers of one subdomain (Failure
// otherwise; mgh_last_error() says so); any supported lossless_type.
enum class target_metric : int { MaxAbs = MGH_TARGET_MAX_ABS, RMSE = MGH_TARGET_RMSE, PSNR = MGH_TARGET_PSNR };
inline compress_status_type achieved_errors(DIM D, data_type dtype, std::vector<SIZE> shape,
                                            const std::vector<double> &tols, double s, error_bound_type mode,
                                            const void *original_data, std::vector<const Byte *> coords,
                                            HighLevelConfig config, std::vector<mgh_error_stats> &stats) {
  if (shape.size() != D) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  stats.assign(tols.size(), mgh_error_stats{});
  return detail::status(mgh_achieved_errors(D, (int)dtype, shape.data(), (int)tols.size(), tols.data(), s, (int)mode,
                                            original_data, cp.empty() ? nullptr : cp.data(), &c, stats.data()));
}
// EXTENSION: mgh_compress_target. The container of the largest tolerance in [tol_min, tol_max] whose achieved
// error meets `target` in `metric` (`rounds` in 1..16 bisections): the container compress(tol_used) writes.
// Failure (MGH_ERR_TARGET_NOT_MET behind it) when not even tol_min meets the target (nothing allocated).
inline compress_status_type compress_target(DIM D, data_type dtype, std::vector<SIZE> shape, target_metric metric,
                                            double target, double tol_min, double tol_max, int rounds, double s,
                                            error_bound_type mode, const void *original_data, void *&compressed_data,
                                            size_t &compressed_size, std::vector<const Byte *> coords,
                                            HighLevelConfig config, bool output_pre_allocated, double &tol_used,
                                            mgh_error_stats *stats_used = nullptr, int *candidates = nullptr) {
  if (shape.size() != D) return compress_status_type::Failure;
  const mgh_config c = detail::to_c(config);
  std::vector<const void *> cp(coords.begin(), coords.end());
  return detail::status(mgh_compress_target(D, (int)dtype, shape.data(), (int)metric, target, tol_min, tol_max, rounds, s,
                                            (int)mode, original_data, &compressed_data, &compressed_size,
                                            cp.empty() ? nullptr : cp.data(), &c, output_pre_allocated ? 1 : 0, &tol_used,
                                            stats_used, candidates));
}
// The figures of the reference's Utilities/ErrorCalculator.h (semantics: mgard_hip_errors.hpp), one pass
// of mgh_compare on `device`; host or device pointers.
template <typename T> double L_inf_norm(size_t n, const T *data, int device = 0) {
  return mgard_hip_errors::L_inf_norm(n, data, device);
}
template <typename T> double L_2_norm(std::vector<SIZE> shape, const T *data, bool normalize_coordinates, int device = 0) {
  return mgard_hip_errors::L_2_norm(mgard_hip_errors::count(shape), data, normalize_coordinates, device);
}
template <typename T>
double L_inf_error(size_t n, const T *original_data, const T *decompressed_data, error_bound_type mode, int device = 0) {
  return mgard_hip_errors::L_inf_error(n, original_data, decompressed_data, mode == error_bound_type::REL, device);
}
template <typename T>
double L_2_error(std::vector<SIZE> shape, const T *original_data, const T *decompressed_data, error_bound_type mode,
                 bool normalize_coordinates, int device = 0) {
  return mgard_hip_errors::L_2_error(mgard_hip_errors::count(shape), original_data, decompressed_data,
                                     mode == error_bound_type::REL, normalize_coordinates, device);
}
template <typename T> double MSE(size_t n, const T *original_data, const T *decompressed_data, int device = 0) {
  return mgard_hip_errors::MSE(n, original_data, decompressed_data, device);
}
template <typename T> double PSNR(size_t n, const T *original_data, const T *decompressed_data, int device = 0) {
  return mgard_hip_errors::PSNR(n, original_data, decompressed_data, device);
}
// ... the box [lo_d, lo_d + ext_d) of it alone (mgh_decompress_preview_window): a dense array of shape ext;
// subdomains the box does not meet are not opened. lo, ext: one entry per dimension of the array.
inline compress_status_type decompress_preview_window(const void *compressed_data, size_t compressed_size, int halvings,
                                                      const std::vector<uint64_t> &lo, const std::vector<uint64_t> &ext,
                                                      void *&decompressed_data, HighLevelConfig config,
                                                      bool output_pre_allocated) {
  const mgh_config c = detail::to_c(config);
  return detail::status(mgh_decompress_preview_window(compressed_data, compressed_size, halvings, lo.data(), ext.data(),
                                                      &decompressed_data, &c, output_pre_allocated ? 1 : 0));
}
// shape of the stitched array and the largest number of halvings; halvings < 0: only the latter
// (shape left empty)
inline compress_status_type infer_coarsened_shape(const void *compressed_data, size_t compressed_size, int halvings,
                                                  HighLevelConfig config, std::vector<SIZE> &shape,
                                                  int &max_halvings) {
  const mgh_config c = detail::to_c(config);
  int D = 0, K = 0;
  uint64_t shp[MGH_MAX_DIM];
  shape.clear();
  const int rc = mgh_infer_coarsened_shape(compressed_data, compressed_size, &c, halvings, &D, shp, &K);
  if (rc != MGH_SUCCESS) return detail::status(rc);
  max_halvings = K;
  if (halvings >= 0) shape.assign(shp, shp + D);
  return compress_status_type::Success;
}
// index in the full array of every node of the stitched grid along `dim` (mgh_infer_coarsened_nodes)
inline compress_status_type infer_coarsened_nodes(const void *compressed_data, size_t compressed_size, int halvings,
                                                  int dim, HighLevelConfig config, std::vector<SIZE> &nodes) {
  const mgh_config c = detail::to_c(config);
  int D = 0;
  uint64_t shp[MGH_MAX_DIM];
  nodes.clear();
  int rc = mgh_infer_shape(compressed_data, compressed_size, &D, shp);
  if (rc != MGH_SUCCESS) return detail::status(rc);
  if (halvings < 0 || dim < 0 || dim >= D) return compress_status_type::Failure;
  std::vector<uint64_t> idx(shp[dim]);
  rc = mgh_infer_coarsened_nodes(compressed_data, compressed_size, &c, halvings, dim, idx.data(), idx.size());
  if (rc < 0) return detail::status(rc);
  nodes.assign(idx.begin(), idx.begin() + rc);
  return compress_status_type::Success;
}
// where the coefficients of `level` lie in a reorder = 1 record (mgh_infer_level_range)
inline compress_status_type infer_level_range(const void *compressed_data, size_t compressed_size, int level,
                                              HighLevelConfig config, SIZE &first_elem, SIZE &num_elems,
                                              SIZE &first_chunk, SIZE &num_chunks) {
  const mgh_config c = detail::to_c(config);
  uint64_t v[4] = {0, 0, 0, 0};
  const int rc = mgh_infer_level_range(compressed_data, compressed_size, &c, level, &v[0], &v[1], &v[2], &v[3]);
  if (rc != MGH_SUCCESS) return detail::status(rc);
  first_elem = v[0];
  num_elems = v[1];
  first_chunk = v[2];
  num_chunks = v[3];
  return compress_status_type::Success;
}
// EXTENSION: a reduced-resolution reconstruction of a reorder = 1 container refined level by level
// (mgh_progressive). The container is borrowed until the reader is destroyed.
class ProgressiveReader {
public:
  ProgressiveReader(const void *compressed_data, size_t compressed_size, HighLevelConfig config = HighLevelConfig()) {
    const mgh_config c = detail::to_c(config);
    check(mgh_progressive_open(&p_, compressed_data, compressed_size, &c), "ProgressiveReader");
  }
  ~ProgressiveReader() { mgh_progressive_close(p_); }
  ProgressiveReader(const ProgressiveReader &) = delete;
  ProgressiveReader &operator=(const ProgressiveReader &) = delete;
  int level() const { return mgh_progressive_level(p_); }  // -1 before the first refine
  // the dense array of to_level (above level()), like decompress_level returns it
  compress_status_type refine(int to_level, void *&data, bool output_pre_allocated) {
    return detail::status(mgh_progressive_refine(p_, to_level, &data, output_pre_allocated ? 1 : 0));
  }
  // the current level prolonged to the container's own grid (mgh_progressive_preview); the state stays
  compress_status_type preview(void *&data, bool output_pre_allocated) {
    return detail::status(mgh_progressive_preview(p_, &data, output_pre_allocated ? 1 : 0));
  }
  // ... the box [lo_d, lo_d + ext_d) of it alone (mgh_progressive_preview_window)
  compress_status_type preview_window(const std::vector<uint64_t> &lo, const std::vector<uint64_t> &ext, void *&data,
                                      bool output_pre_allocated) {
    return detail::status(mgh_progressive_preview_window(p_, lo.data(), ext.data(), &data, output_pre_allocated ? 1 : 0));
  }

private:
  mgh_progressive *p_ = nullptr;
};
// EXTENSION: the stateful reader of precision layers (mgh_layers): layer 0 at construction, then add() per
// layer in the writer's order, data() whenever an array is wanted. The containers are not kept.
class LayersReader {
public:
  LayersReader(const void *layer0, size_t size, HighLevelConfig config = HighLevelConfig()) {
    const mgh_config c = detail::to_c(config);
    check(mgh_layers_open(&p_, layer0, size, &c), "LayersReader");
  }
  ~LayersReader() { mgh_layers_close(p_); }
  LayersReader(const LayersReader &) = delete;
  LayersReader &operator=(const LayersReader &) = delete;
  int count() const { return mgh_layers_count(p_); }
  double tolerance() const { return mgh_layers_tolerance(p_); }
  compress_status_type add(const void *layer, size_t size) { return detail::status(mgh_layers_add(p_, layer, size)); }
  compress_status_type data(void *&out, bool output_pre_allocated) {
    return detail::status(mgh_layers_data(p_, &out, output_pre_allocated ? 1 : 0));
  }
  // (mgh_layers_data_level: the array of `level` of the hierarchy only)
  compress_status_type data(int level, void *&out, bool output_pre_allocated) {
    return detail::status(mgh_layers_data_level(p_, level, &out, output_pre_allocated ? 1 : 0));
  }

private:
  mgh_layers *p_ = nullptr;
};
// EXTENSION: the stateful reader of precision layers in level order (mgh_level_layers): layer 0 up to `level`
// at construction, add() the next layer up to a level, extend() a layer deeper, data(level) whenever an
// array is wanted. depth(k) never exceeds depth(k - 1); data needs level <= depth(0).
class LevelLayersReader {
public:
  LevelLayersReader(const void *layer0, size_t size, int level, HighLevelConfig config = HighLevelConfig()) {
    const mgh_config c = detail::to_c(config);
    check(mgh_level_layers_open(&p_, layer0, size, &c, level), "LevelLayersReader");
  }
  ~LevelLayersReader() { mgh_level_layers_close(p_); }
  LevelLayersReader(const LevelLayersReader &) = delete;
  LevelLayersReader &operator=(const LevelLayersReader &) = delete;
  int count() const { return mgh_level_layers_count(p_); }
  int depth(int k) const { return mgh_level_layers_depth(p_, k); }
  double tolerance(int k) const { return mgh_level_layers_tolerance(p_, k); }
  compress_status_type add(const void *layer, size_t size, int level) {
    return detail::status(mgh_level_layers_add(p_, layer, size, level));
  }
  compress_status_type extend(int k, const void *layer, size_t size, int level) {
    return detail::status(mgh_level_layers_extend(p_, k, layer, size, level));
  }
  compress_status_type data(int level, void *&out, bool output_pre_allocated) {
    return detail::status(mgh_level_layers_data(p_, level, &out, output_pre_allocated ? 1 : 0));
  }

private:
  mgh_level_layers *p_ = nullptr;
};
inline compress_status_type decompress(const void *compressed_data, size_t compressed_size,
                                       void *&decompressed_data, std::vector<SIZE> &shape,
                                       data_type &dtype, HighLevelConfig config, bool output_pre_allocated) {
  int D = 0, dt = 0;
  uint64_t shp[MGH_MAX_DIM];
  int rc = mgh_infer_shape(compressed_data, compressed_size, &D, shp);
  if (rc == MGH_SUCCESS) rc = mgh_infer_data_type(compressed_data, compressed_size, &dt);
  if (rc != MGH_SUCCESS) return detail::status(rc);
  shape.assign(shp, shp + D);
  dtype = dt == MGH_DOUBLE ? data_type::Double : data_type::Float;
  return decompress(compressed_data, compressed_size, decompressed_data, config, output_pre_allocated);
}
inline compress_status_type decompress(const void *compressed_data, size_t compressed_size,
                                       void *&decompressed_data, std::vector<SIZE> &shape,
                                       data_type &dtype, bool output_pre_allocated) {
  return decompress(compressed_data, compressed_size, decompressed_data, shape, dtype, HighLevelConfig(),
                    output_pre_allocated);
}

// The remaining stages of the reference's LOW-LEVEL Compressor (Compressor.h:39-78):
// LosslessCompress + Serialize, Deserialize + LosslessDecompress, and Compress / Decompress that
// chain all stages (Compressor.hpp:193-272). The serialized record is the subdomain payload of
// the container (Huffman.hpp:163-239); it lives in host memory owned by this object.
template <DIM D, typename T> class LosslessCompressor {
public:
  explicit LosslessCompressor(Compressor<D, T> &c, HighLevelConfig config = HighLevelConfig())
      : c_(&c), config_(config) {
    check(mgh_lossless_create(&ctx_, config.dev_id), "LosslessCompressor");
  }
  ~LosslessCompressor() { mgh_lossless_destroy(ctx_); }
  LosslessCompressor(const LosslessCompressor &) = delete;
  LosslessCompressor &operator=(const LosslessCompressor &) = delete;

  // LosslessCompress + Serialize: quantized_array() and the outlier list of the Compressor ->
  // record bytes (valid until the next call)
  void LosslessCompress(SIZE n, SIZE outlier_count, const Byte *&data, SIZE &size, void *queue = nullptr) {
    const uint8_t *p = nullptr;
    uint64_t sz = 0;
    check(mgh_lossless_compress(ctx_, c_->quantized_array(), n, config_.huff_dict_size,
                                config_.huff_block_size, (int)config_.lossless,
                                config_.zstd_compress_level, c_->outlier_indexes(), c_->outliers(),
                                outlier_count, &p, &sz, queue),
          "LosslessCompress");
    data = p;
    size = sz;
  }
  // Deserialize + LosslessDecompress: record bytes -> quantized_array(); the outlier list comes
  // back in device buffers owned by this object
  void LosslessDecompress(const Byte *data, SIZE size, SIZE n, const ATOMIC_IDX *&outlier_idx,
                          const QUANTIZED_INT *&outliers, SIZE &outlier_count, void *queue = nullptr) {
    uint64_t cnt = 0;
    check(mgh_lossless_decompress(ctx_, data, size, (int)config_.lossless, c_->quantized_array(), n,
                                  &outlier_idx, &outliers, &cnt, queue),
          "LosslessDecompress");
    outlier_count = cnt;
  }
  // ... of the chunks that hold integers [first, first + count) only, into `out` (mgh_lossless_decompress_range)
  void LosslessDecompressRange(const Byte *data, SIZE size, SIZE n, SIZE first, SIZE count, QUANTIZED_INT *out,
                               const ATOMIC_IDX *&outlier_idx, const QUANTIZED_INT *&outliers, SIZE &outlier_count,
                               void *queue = nullptr) {
    uint64_t cnt = 0;
    check(mgh_lossless_decompress_range(ctx_, data, size, (int)config_.lossless, out, n, first, count, &outlier_idx,
                                        &outliers, &cnt, queue),
          "LosslessDecompressRange");
    outlier_count = cnt;
  }

private:
  Compressor<D, T> *c_;
  HighLevelConfig config_;
  mgh_lossless_ctx *ctx_ = nullptr;
};

// release_cache (compress_x.hpp:159)
inline compress_status_type release_cache(HighLevelConfig = HighLevelConfig()) {
  mgh_release_cache();
  return compress_status_type::Success;
}

} // namespace mgard_hip

#endif // COMPRESS_HIP_HPP
