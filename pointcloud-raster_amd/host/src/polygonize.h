// polygonize.h -- (internal) the zones of a band of memory as a PolygonSet: what pcr::polygonize and Pipeline::polygonize share.
// The rule is csrc/polygonize.hpp; the contract is in include/pcr_hip.h ("polygonize").
#pragma once

#include "../../csrc/polygonize.hpp"
#include "buffer.h"
#include "pcr/core/polygons.h"
#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"

namespace pcr {
namespace detail {

/// `band`: geometry.height rows of geometry.width floats, contiguous, in `loc` memory.  Host: polygonize.hpp's sequential trace.
/// Device: the C-ABI's kernels on `stream` with work areas of the call's own, released after waiting for the stream; the ring
/// table alone is copied out.  Then ONE pass over the table: the rings grouped by zone (stable) and the corners placed.
Status polygonize_band(const float* band, const GridConfig& geometry, MemoryLocation loc, void* stream, PolygonSet* out);

/// Pipeline::polygonize's refusals, the same on both engines; `band`: the index of `band_name` in `result`.
Status polygonize_check(const PipelineConfig& cfg, const PolygonSet* out, bool fresh, const Grid* result, const std::string& band_name,
                        int* band);

}  // namespace detail
}  // namespace pcr
