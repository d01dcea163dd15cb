// jds_xform_dev.hpp — the launch interface of the coefficient transform
// (jds_xform.hip) as the C-ABI sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_xform.hpp"

namespace jds {

// One launch over the ntiles tiles of all records: tilefile[t] = the record of
// tile t.  src and dst are the bases the records' offsets count from (they may
// be one allocation: a record's source and destination planes do not overlap).
hipError_t launch_coef_xform(const XfFile* files, const int32_t* tilefile, long long ntiles, const int16_t* src,
                             int16_t* dst, hipStream_t s);

}  // namespace jds
