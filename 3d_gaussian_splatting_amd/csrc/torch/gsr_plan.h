// gsr_plan.h -- the partition arithmetic of the multi-GPU step: which Gaussians a
// rank owns, where the bands of tile rows are cut, and how large the exchange and binning
// capacities must be.  Pure integer / double host code, the C++ twin of bands.py: this header and
// gsr_plan.cpp include the C++ standard library only (tests/test_multiprocess.py compiles them
// with nothing else on the include path).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace gsr {

inline int64_t round_up(int64_t x, int64_t m = 256) { return (x + m - 1) / m * m; }

// A capacity for `need` items: round_up(ceil(max(need, 1) x headroom)).
int64_t capacity_with_headroom(int64_t need, double headroom);
// The C ABI counts in int32: throws std::overflow_error when the band capacity, or the `world`
// blocks of pair_cap splats a band receives, reach INT32_MAX.
void require_int32_capacities(int64_t pair_cap, int64_t capacity, int world);

std::pair<int64_t, int64_t> gaussian_shard(int64_t P, int world, int rank);
std::vector<int> equal_bands(int grid_y, int world);
std::vector<int> balance_bands(const std::vector<int64_t>& row_counts, int world);

// Band cuts and capacities from one step's statistics (GSR_FLAG_ROW_SPANS of every shard, summed
// or per shard): inst[y] = instances in tile row y over all shards; starts[s][y] / ends[s][y] =
// shard s's visible Gaussians whose rect's first / last tile row is y.  The splats shard s sends
// to band [r0, r1) are exactly sum_{y<r1} starts[s][y] - sum_{y<r0} ends[s][y], so the needed
// pair_cap and band capacity (before headroom) follow for any cuts.  Same arithmetic as
// bands.plan_from_stats.
struct StatsPlan {
    std::vector<int> rows;
    int64_t max_splats = 0;  // largest (shard, band) splat count under `rows`
    std::vector<int64_t> band_k;
};
StatsPlan plan_from_stats(const std::vector<int64_t>& inst, const std::vector<std::vector<int64_t>>& starts,
                          const std::vector<std::vector<int64_t>>& ends, int world);

}  // namespace gsr
