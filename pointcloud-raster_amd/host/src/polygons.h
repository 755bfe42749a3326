// polygons.h -- (internal) a PolygonSet burnt into a band of memory that already exists: what rasterize_polygons and
// Pipeline::set_zones(name, polygons) share.  The arithmetic is csrc/rasterize.hpp; the contract is in include/pcr_hip.h
// ("polygons").
#pragma once

#include "../../csrc/rasterize.hpp"
#include "buffer.h"
#include "pcr/core/polygons.h"
#include "pcr_hip.h"

namespace pcr {
namespace detail {

/// `dst`: geometry.height rows of geometry.width floats, contiguous, in `loc` memory.  Host: the C-ABI's host twin.  Device: the
/// kernels on `stream` with a work area of the call's own, which is released after waiting for the stream.
Status rasterize_into(const PolygonSet& set, const GridConfig& geometry, const RasterizeOptions& options, float* dst,
                      MemoryLocation loc, void* stream);

}  // namespace detail
}  // namespace pcr
