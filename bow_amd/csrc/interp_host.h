// interp_host.h — what the host files of Rolling.Interpolate hand each other: interpolate_api.cpp (validation, pass 1, the fill and
// the entry points) and interp_null_ts.cpp (the call over an interval column with nulls, which runs the ordinary count and fill on its
// compacted rows).  Host only: no .hip file and not common.h includes it.
#pragma once

#include "common.h"

namespace bowgpu {

// interpolate_api.cpp: the ordinary count and fill.  global_s0 + edge: a row-range shard (nullptr: the whole frame)
int interp_count_impl(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                      const bowgpu_interp *interps, int32_t ninterps, int64_t *n_out, const int64_t *global_s0, const bowgpu_interp_edge *edge);
int interp_fill_impl(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                     const bowgpu_interp *interps, int32_t ninterps, bowgpu_out *outs, const int64_t *global_s0, const bowgpu_interp_edge *edge);
// interp_null_ts.cpp: the call when the interval column has nulls, a Bow of any width.  outs == nullptr: the row count only;
// *applies = false: the column has none and nothing was done
int interp_null_ts_any(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                       const bowgpu_interp *interps, int32_t ninterps, int64_t *n_out, bowgpu_out *outs, bool *applies);

}  // namespace bowgpu
