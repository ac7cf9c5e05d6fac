// The layout of the two small blocks every thread context owns, stated once: the SCRATCH block in device memory (ctx_scratch) and the
// REGISTERED block, pinned host memory that kernels store results into themselves (ctx_pinned).  Plain constants for host and device
// code.  common.h includes this file behind the constants that bound the regions (kStatusWords, kMaxAggs, kMaxCols, kMoveCols,
// kConvertShards, kInterpEdgeBlocks, kShardMaxWorld) and puts the two accessors, scratch_at / registered_at, next to it.
//
// One thread runs one entry point at a time, so regions of different entry points overlap freely.  What may NOT overlap are regions
// that hold data at the same time: a call's own, and those of the helpers it calls while its own are live.  Each such set is one
// all_apart() assert below; a region that is read back before the next one is written (the Sort histogram before the move groups,
// the Interpolate count pass before the fill) is deliberately in no set with it.
#pragma once

#include <stddef.h>

#include "../../include/bowgpu.h"

namespace bowgpu {

struct Region {
    size_t offset, size;   // bytes
    constexpr size_t end() const { return offset + size; }
};
constexpr bool apart(Region a, Region b) { return a.end() <= b.offset || b.end() <= a.offset; }
constexpr bool all_apart() { return true; }
template <class... R> constexpr bool all_apart(Region a, R... rest) { return (apart(a, rest) && ...) && all_apart(rest...); }   // every pair
constexpr bool inside(size_t bytes) { return true; }
template <class... R> constexpr bool inside(size_t bytes, Region a, R... rest) { return a.end() <= bytes && inside(bytes, rest...); }
// bytes from the start of `first` to the end of `last`: what one memset / one copy over both (and the gap between them) covers
constexpr size_t span(Region first, Region last) { return last.end() - first.offset; }

// ================================================================ the scratch block (device)
// region                                                             owner; lives
constexpr Region kScrStatus = {0, 4 * (size_t)kStatusWords};       // status words of whichever call runs (kAggSt*, Interpolate's own meanings); from its zeroing to its read-back
constexpr size_t kStatusHeadBytes = 4 * (size_t)kLongCountWord;    // ... the words in front of the tile pass' sub-list counts: what every other user zeroes
constexpr Region kScrAggCounts = {1024, 8 * (size_t)kMaxAggs};     // tile pass (agg_pass.cpp): valid bits per output bitmap; preset launch to read-back
constexpr Region kScrLongList = {8192, 0};                         // tile pass: the long-window list, sized per call (scr_long_list) - the one region behind the fixed part
constexpr Region kScrInterpCounts = {1024, 8 * (size_t)kMaxCols};  // Interpolate fill through working copies: valid rows per column of a batch; one batch
constexpr Region kScrOneCount = {1024, 8};                         // Parquet column read, recount_nulls: one count of valid rows; one call
constexpr Region kScrOrderFlags = {256, 4};                        // col_order_flags (IsColSorted, FillLinear): one word; inside the helper
constexpr Region kScrFillFar = {0, 4};                             // fill_finish: "a neighbour lies further than the walk"; one attempt
constexpr Region kScrFillCount = {8, 8};                           // fill_finish: valid outputs; one attempt
constexpr Region kScrNullCount = {2048, 8};                        // count_nulls_device - a HELPER, run by devcol_prepare inside most calls; inside the helper
constexpr Region kScrProbe = {3072, 16};                           // stream probes, checksum (runtime.cpp): two 64-bit words; one call
constexpr Region kScrConvertCounts = {0, 8 * (size_t)kMoveCols * kConvertShards};   // Convert: valid rows per column and shard; one group
constexpr Region kScrHist = {0, 8 * 256 * 4};                      // Sort: [8][256] digit counts; inside argsort_device (read back before it returns)
constexpr Region kScrFlags = {8192, 16};                           // four words.  Sort: [0] not ascending, [1] NaN seen, [2] bad index (take); Filter: filter_stats_kernel's; Find: the row
constexpr Region kScrEqualWord = {8192, 8};                         // Equal: (row << 32) | column of the first difference, kept across the launch groups of a call (lies in kScrFlags: one call at a time)
constexpr Region kScrMoveCounts = {8208, 8 * (size_t)kMoveCols};   // a move group: the outputs' nulls (gather) / valid rows (scatter, append, diff); one group
constexpr Region kScrImages = {0, 8 * (2 * (size_t)kShardMaxWorld + 2)};   // sharded Sort read_images: one image per position; inside the helper
constexpr Region kScrSplitBounds = {0, 4 * 2 * (size_t)kShardMaxWorld};    // sharded Sort splitters: two row counts per candidate; one round
constexpr Region kScrDiag = {0, kScrLongList.offset};              // bowgpu_debug_status: the words a diagnostic build may read and clear

// The fixed part: every region but the long-window list.  ctx_scratch never allocates less, so the block is allocated by a thread's
// first use and only a tile pass whose list needs more can replace it - at the start of that call, before anything points into it.
constexpr size_t kScrFixedBytes = kScrMoveCounts.end();
constexpr Region scr_long_list(size_t bytes) { return {kScrLongList.offset, bytes}; }

// live together: a tile pass and the null counts of the columns staged under it
static_assert(all_apart(kScrStatus, kScrAggCounts, kScrNullCount, scr_long_list(1)), "tile pass");
static_assert(kScrFixedBytes >= kScrLongList.offset, "the fixed part covers everything in front of the list");
// ... Interpolate's fill (its columns are staged after the status words are handed out)
static_assert(all_apart(kScrStatus, kScrInterpCounts, kScrNullCount), "Interpolate fill");
static_assert(kStatusHeadBytes <= kScrStatus.size && kScrInterpCounts.offset == kScrAggCounts.offset, "preset_bitmaps_kernel serves both");
// ... Fill / FillLinear: the order flags are read back before the fill starts, the columns are staged before either; stated anyway
static_assert(all_apart(kScrFillFar, kScrFillCount, kScrOrderFlags, kScrNullCount), "Fill");
static_assert(span(kScrFillFar, kScrFillCount) == 16, "one memset and one copy over the far flag and the count");
// ... a Parquet column read (recount_nulls uses the count alone)
static_assert(all_apart(kScrStatus, kScrOneCount, kScrNullCount), "column read");
// ... Convert (its columns are staged uncounted: the null count does not run under it today)
static_assert(all_apart(kScrConvertCounts, kScrNullCount), "Convert");
// ... a move group of Sort / Filter / Append / Diff / Find, the Filter statistics, and the null counts of the columns staged meanwhile.
// The Sort histogram is NOT in this set: argsort_device has read it back before the first column of a group is staged, and the null
// count lies inside it
static_assert(all_apart(kScrFlags, kScrMoveCounts, kScrNullCount), "move group");
static_assert(kScrEqualWord.offset % 8 == 0 && all_apart(kScrEqualWord, kScrNullCount), "Equal: a 64-bit atomic word");
static_assert(kScrFlags.offset == kScrHist.end() && kScrMoveCounts.offset == kScrFlags.end(), "one memset / one copy over histogram + flags, over flags + counts");
static_assert(inside(kScrFixedBytes, kScrStatus, kScrAggCounts, kScrInterpCounts, kScrOneCount, kScrOrderFlags, kScrFillFar, kScrFillCount, kScrNullCount,
                     kScrProbe, kScrConvertCounts, kScrHist, kScrFlags, kScrEqualWord, kScrMoveCounts, kScrImages, kScrSplitBounds, kScrDiag), "inside the fixed part");

// ================================================================ the registered block (host)
constexpr size_t kRegBytes = 16384;                                // allocated once per thread, never moved
constexpr int kWholeMaxAggs = 64;                                  // whole-frame Aggregate: reducers per call (its slots below)
// region                                                             owner; lives
constexpr Region kRegStatus = {0, 4 * (size_t)kStatusWords};       // tile pass: the status words (finish_bitmaps_kernel's stores, or a copy); Interpolate fill in place: their head.  Until the settle has read them
constexpr Region kRegAggCounts = {1024, 8 * (size_t)kMaxAggs};     // tile pass: valid bits per output bitmap, by the same store / copy
constexpr Region kRegFilterStats = {0, 12};                        // Filter: selected rows, first, last - filter_stats_kernel's stores; mask pass
constexpr Region kRegFindRow = {32, 4};                            // Find: the row, find_result_kernel's store; one call
constexpr Region kRegEqualWord = {40, 8};                          // Equal: the word, equal_result_kernel's store; one call
constexpr Region kRegTwoTs = {2048, 16};                           // plan_make - a HELPER of every windowed call - and whole-frame Aggregate's second implementation: first / last timestamp; inside the helper
constexpr Region kRegInterpCount = {3072, 24};                     // Interpolate count pass: total, two packed status pairs; inside interp_prepare
constexpr Region kRegInterpCounts = {1024, 8 * (size_t)kMaxCols * kInterpEdgeBlocks};   // Interpolate fill in place: partial valid counts, interp_edge_fix_kernel's stores; one batch
constexpr Region kRegSeeds = {4096, sizeof(bowgpu_carry_state) * BOWGPU_CARRY_MAX_AGGS};   // shard finish: the carry seeds on their way to the device; until the finish has synchronised
constexpr Region kRegWholeValues = {8192, 8 * (size_t)kWholeMaxAggs};   // whole-frame Aggregate: one value per reducer, the finish launches' stores; one call
constexpr Region kRegWholeValid = {kRegWholeValues.end(), (size_t)kWholeMaxAggs};   // ... and one validity byte
constexpr Region kRegTailReport = {12288, BOWGPU_CARRY_MAX_AGGS};  // sharded Aggregate's tail: one byte per device-resident output, shard_tail_kernel's stores; inside sharded_tail

// live together: a rank of the sharded Aggregate - the settle of its pass, the seeds of its finish, its tail - and the plan of a call
// made while a pass is in flight
static_assert(all_apart(kRegStatus, kRegAggCounts, kRegTwoTs, kRegSeeds, kRegTailReport), "tile pass, shard finish, tail");
static_assert(kRegStatus.offset == kScrStatus.offset && kRegAggCounts.offset == kScrAggCounts.offset && kRegStatus.size == kScrStatus.size,
              "the read-back is one copy of the scratch block's head, or finish_bitmaps_kernel's stores to the same places");
// ... Interpolate's fill in place.  Its count pass (kRegInterpCount) and the plan (kRegTwoTs) lie INSIDE the partial counts: both are
// consumed inside interp_prepare, which runs before the first batch and - for a redo - after the last batch's counts have been summed
static_assert(all_apart(kRegStatus, kRegInterpCounts), "Interpolate fill");
static_assert(kRegInterpCounts.offset == kScrInterpCounts.offset, "status words and counts arrive in one copy where they are not stored in place");
// ... whole-frame Aggregate
static_assert(all_apart(kRegTwoTs, kRegWholeValues, kRegWholeValid), "whole-frame Aggregate");
static_assert(inside(kRegBytes, kRegStatus, kRegAggCounts, kRegFilterStats, kRegFindRow, kRegEqualWord, kRegTwoTs, kRegInterpCount, kRegInterpCounts, kRegSeeds,
                     kRegWholeValues, kRegWholeValid, kRegTailReport), "inside the block");

// the tile pass' read-back: status words and counts in ONE copy, or stored by finish_bitmaps_kernel, which is handed kRegStatus alone
constexpr size_t kAggCountsFromStatus = kRegAggCounts.offset - kRegStatus.offset;
constexpr size_t kReadbackBytes = span(kScrStatus, kScrAggCounts);

}  // namespace bowgpu
