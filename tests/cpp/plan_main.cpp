// plan_main.cpp -- gsr_plan.cpp alone, with no torch or HIP: the partition arithmetic of the
// multi-GPU step read from stdin and printed, for tests/test_multiprocess.py to compare with
// bands.py.  One case per line of input, one line of output each:
//   shard P world rank                          -> g0 g1
//   equal grid_y world                          -> rows
//   balance world grid_y c[grid_y]              -> rows
//   plan world grid_y shards inst[grid_y] {starts[grid_y] ends[grid_y]} x shards
//                                               -> rows | max_splats | band_k
#include <iostream>
#include <string>
#include <vector>

#include "gsr_plan.h"

template <class T>
static std::vector<T> read_n(int n) {
    std::vector<T> v(n);
    for (auto& x : v) std::cin >> x;
    return v;
}

template <class V>
static void print(const V& v, const char* end) {
    for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? " " : "") << v[i];
    std::cout << end;
}

int main() {
    std::string op;
    while (std::cin >> op) {
        if (op == "shard") {
            int64_t P;
            int world, rank;
            std::cin >> P >> world >> rank;
            const auto r = gsr::gaussian_shard(P, world, rank);
            std::cout << r.first << " " << r.second << "\n";
        } else if (op == "equal") {
            int gy, world;
            std::cin >> gy >> world;
            print(gsr::equal_bands(gy, world), "\n");
        } else if (op == "balance") {
            int world, gy;
            std::cin >> world >> gy;
            print(gsr::balance_bands(read_n<int64_t>(gy), world), "\n");
        } else if (op == "plan") {
            int world, gy, shards;
            std::cin >> world >> gy >> shards;
            const auto inst = read_n<int64_t>(gy);
            std::vector<std::vector<int64_t>> starts, ends;
            for (int s = 0; s < shards; ++s) {
                starts.push_back(read_n<int64_t>(gy));
                ends.push_back(read_n<int64_t>(gy));
            }
            const gsr::StatsPlan sp = gsr::plan_from_stats(inst, starts, ends, world);
            print(sp.rows, " | ");
            std::cout << sp.max_splats << " | ";
            print(sp.band_k, "\n");
        } else {
            std::cerr << "unknown case " << op << "\n";
            return 2;
        }
        if (!std::cin) {
            std::cerr << "truncated case " << op << "\n";
            return 2;
        }
    }
    return 0;
}
