// pcr/core/reproject.h -- coordinate reprojection between the CRSs the C-ABI knows (include/pcr_hip.h,
// pcr_hip_crs_from_epsg): WGS 84 / NAD83 / ETRS89 geographic, Web Mercator, and the UTM zones on those datums, which are
// treated as one datum (no datum shift).  Not in the reference, which declares PipelineConfig::target_crs and
// auto_reproject but never reads them; here Pipeline::ingest reprojects a cloud whose CRS differs from the grid's.
#pragma once

#include "pcr/core/types.h"

#include <cstddef>

namespace pcr {

class PointCloud;

/// EPSG code of a CRS: CRS::epsg when set, else the top-level authority of its WKT (the last AUTHORITY["EPSG","n"] of the
/// outermost node in WKT1, ID["EPSG",n] in WKT2; a nested GEOGCS authority does not count).  0: unidentified.
int crs_epsg(const CRS& crs);

/// Transforms n points from `src` to `dst`.  The arrays live in `loc` (Host and HostPinned: on the calling thread's CPUs;
/// Device: on the device, synchronously).  ox / oy are x / y themselves (in place) or do not overlap them.  Points
/// outside the domain become NaN.  CrsError when either CRS is unidentified or not supported.
Status transform_xy(const CRS& src, const CRS& dst, const double* x, const double* y, double* ox, double* oy, size_t n,
                    MemoryLocation loc);

/// Reprojects the cloud's coordinates in place (wherever it lives) and sets its CRS to `dst`.
Status reproject(PointCloud& cloud, const CRS& dst);

}  // namespace pcr
