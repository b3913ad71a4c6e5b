// Drives eqf_vio_amd/csrc/eqf_mergecost_host.hpp (host only, standard library only) for tests/test_mergecost_host.py: one case per line on
// stdin, results on stdout (doubles as hexadecimal floats).  Built with g++ under the address and undefined-behaviour sanitizers; every
// buffer is a std::vector of exactly the size the header is told about, so an index one past an end is a report, not a silent read.
//   args n kind first npairs null pairs[2 npairs]   (null 1: pairs == NULL)        -> 0 | 1
//   lex n                                           -> every pair "i j" of the enumeration
//   items n kind npairs null idx[n] w~[n] pairs[..] -> per item "i j bi bj self alpha wi wj"
//   distinct B n idx[n]                             -> the distinct filters
//   plan items option B                             -> chunk, number of chunks, then the count of every chunk
//   order N first                                   -> offset, padded order, block columns, launches per chunk
//   cost kind ldi ldj ldij maha wi wj               -> alpha, cost
//   option value                                    -> 0 | 1
//   work C sigmaStride nTot dRec head glob          -> offW offE offD offOut offGlob offBad doubles   (all in doubles)
//   itemblock itemCap                               -> offItems offRecords bytes sizeof(Item)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_mergecost_host.hpp"

using namespace eqf::mergecost;

static double readDouble(std::istringstream& in) {
    std::string t;
    in >> t;
    return std::stod(t);  // ("nan", "inf", "-inf" and hexadecimal floats included)
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "args") {
            int n, kind, first, npairs, null;
            in >> n >> kind >> first >> npairs >> null;
            std::vector<int> pairs(npairs > 0 && !null ? 2 * size_t(npairs) : 0);
            for (auto& v : pairs) in >> v;
            static const int none = 0;
            const int* pp = null ? nullptr : (pairs.empty() ? &none : pairs.data());
            std::printf("%d\n", pairArgsOk(n, kind, first, npairs, pp) ? 1 : 0);
        } else if (cmd == "lex") {
            int n;
            in >> n;
            for (long long p = 0; p < allPairs(n); ++p) {
                int i, j;
                lexPair(n, p, &i, &j);
                std::printf("%d %d ", i, j);
            }
            std::printf("\n");
        } else if (cmd == "items") {
            int n, kind, npairs, null;
            in >> n >> kind >> npairs >> null;
            std::vector<int> idx(n), pairs(null ? 0 : 2 * size_t(npairs));
            std::vector<double> wt(n);
            for (auto& v : idx) in >> v;
            for (auto& v : wt) v = readDouble(in);
            for (auto& v : pairs) in >> v;
            std::vector<Item> items;
            buildItems(n, idx.data(), wt.data(), kind, npairs, null ? nullptr : pairs.data(), items);
            for (const Item& t : items) std::printf("%d %d %d %d %d %a %a %a ", t.i, t.j, t.bi, t.bj, t.self, t.alpha, t.wi, t.wj);
            std::printf("\n");
        } else if (cmd == "distinct") {
            int B, n;
            in >> B >> n;
            std::vector<int> idx(n), uniq;
            for (auto& v : idx) in >> v;
            distinct(n, idx.data(), B, uniq);
            for (int u : uniq) std::printf("%d ", u);
            std::printf("\n");
        } else if (cmd == "plan") {
            long long items;
            int option, B;
            in >> items >> option >> B;
            const int chunk = chunkSize(option, B), nc = numChunks(items, chunk);
            std::printf("%d %d ", chunk, nc);
            for (int c = 0; c < nc; ++c) std::printf("%d ", chunkCount(items, chunk, c));
            std::printf("\n");
        } else if (cmd == "order") {
            int N, first;
            in >> N >> first;
            const int off = offsetOf(first), m = paddedOrder(N, off);
            std::printf("%d %d %d %d\n", off, m, blockColumns(m), launchesPerChunk(m));
        } else if (cmd == "cost") {
            int kind;
            in >> kind;
            double v[6];
            for (double& x : v) x = readDouble(in);
            const double a = alphaOf(kind, v[4], v[5]);
            std::printf("%a %a\n", a, cost(kind, v[0], v[1], v[2], v[3], v[4], v[5], a));
        } else if (cmd == "work") {
            size_t v[6];
            for (size_t& x : v) in >> x;
            const WorkLayout w{v[0], v[1], v[2], v[3], v[4], v[5]};
            std::printf("%zu %zu %zu %zu %zu %zu %zu\n", w.offW(), w.offE(), w.offD(), w.offOut(), w.offGlob(), w.offBad(), w.doubles());
        } else if (cmd == "itemblock") {
            size_t cap;
            in >> cap;
            const ItemsLayout l{cap};
            std::printf("%zu %zu %zu %zu\n", l.offItems(), l.offRecords(), l.bytes(), sizeof(Item));
        } else if (cmd == "option") {
            int value;
            in >> value;
            std::printf("%d\n", chunkOptionOk(value) ? 1 : 0);
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
