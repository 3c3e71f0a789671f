// gsr_plan.cpp -- the partition arithmetic of the multi-GPU step: the same arithmetic as bands.py
// (see gsr_plan.h).  Standard library only.
#include "gsr_plan.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace gsr {

int64_t capacity_with_headroom(int64_t need, double headroom) {
    return round_up((int64_t)std::ceil(std::max<int64_t>(need, 1) * headroom));
}

void require_int32_capacities(int64_t pair_cap, int64_t capacity, int world) {
    if (capacity >= INT32_MAX || pair_cap * world >= INT32_MAX)
        throw std::overflow_error("ShardStep: band capacity / pair_cap exceed int32: use more ranks");
}

std::pair<int64_t, int64_t> gaussian_shard(int64_t P, int world, int rank) {
    const int64_t S = (P + world - 1) / world;
    return {std::min<int64_t>(rank * S, P), std::min<int64_t>((int64_t)(rank + 1) * S, P)};
}

std::vector<int> equal_bands(int grid_y, int world) {
    std::vector<int> r(world + 1);
    for (int i = 0; i <= world; ++i) r[i] = (int)((int64_t)i * grid_y / world);
    return r;
}

std::vector<int> balance_bands(const std::vector<int64_t>& c, int world) {
    const int gy = (int)c.size();
    if (world > gy) throw std::invalid_argument("balance_bands: more bands than tile rows");
    std::vector<double> pre(gy + 1, 0.0);
    for (int i = 0; i < gy; ++i) pre[i + 1] = pre[i] + (double)c[i];
    const double total = pre[gy];
    if (total <= 0) return equal_bands(gy, world);
    std::vector<int> rows{0};
    for (int k = 1; k < world; ++k) {
        const double t = k * total / world;
        int y = 0;
        double best = std::fabs(pre[0] - t);
        for (int i = 1; i <= gy; ++i)  // first index of the minimum, as numpy.argmin
            if (std::fabs(pre[i] - t) < best) best = std::fabs(pre[i] - t), y = i;
        y = std::max(y, rows.back() + 1);
        y = std::min(y, gy - (world - k));
        rows.push_back(y);
    }
    rows.push_back(gy);
    return rows;
}

StatsPlan plan_from_stats(const std::vector<int64_t>& inst, const std::vector<std::vector<int64_t>>& starts,
                          const std::vector<std::vector<int64_t>>& ends, int world) {
    const int gy = (int)inst.size();
    StatsPlan sp;
    sp.rows = balance_bands(inst, world);
    sp.band_k.assign(world, 0);
    for (int b = 0; b < world; ++b)
        for (int y = sp.rows[b]; y < sp.rows[b + 1]; ++y) sp.band_k[b] += inst[y];
    for (size_t s = 0; s < starts.size(); ++s) {
        std::vector<int64_t> ps(gy + 1, 0), pe(gy + 1, 0);  // prefix sums of starts / ends
        for (int y = 0; y < gy; ++y) ps[y + 1] = ps[y] + starts[s][y], pe[y + 1] = pe[y] + ends[s][y];
        for (int b = 0; b < world; ++b)
            sp.max_splats = std::max(sp.max_splats, ps[sp.rows[b + 1]] - pe[sp.rows[b]]);
    }
    return sp;
}

}  // namespace gsr
