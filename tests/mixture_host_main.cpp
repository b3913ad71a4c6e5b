// Drives eqf_vio_amd/csrc/eqf_mixture_host.hpp (host only, standard library only) for tests/test_mixture_host.py: one case per line on stdin,
// results on stdout (doubles as hexadecimal floats).  Built with g++ under the address and undefined-behaviour sanitizers; every buffer is
// a std::vector of exactly the size the header is told about, so an index one past an end is a report, not a silent read.
//   grid N                       -> refOrder paddedOrder chunks rowBlocks (the launch grid of k_mix_reduce)
//   map N                        -> the padded index of every reference index
//   layout B cap ld globWords    -> jacStride estStride offJac offEst offErr offMean offOut offP0 offQ offGlob offVerdict doubles
//   head B ref n idx[n] w[n] null  (null 0 none | 1 idx | 2 w; a weight "nan" / "inf" is read as such)   -> 0 | 1
//   ids na a[na] nb b[nb]        -> 0 | 1
//   norm n w[n]                  -> n_eff, then w~[n]
//   tables B ref n idx[n] w[n]   -> the members "b w~" in walking order, then the distinct filters
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_mixture_host.hpp"

using namespace eqf::mixture;

static double readDouble(std::istringstream& in) {
    std::string t;
    in >> t;
    return std::stod(t);  // ("nan", "inf", "-inf" included)
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "grid") {
            int N;
            in >> N;
            std::printf("%d %d %d %d\n", refOrder(N), paddedOrder(N), chunks(N), rowBlocks(N));
        } else if (cmd == "map") {
            int N;
            in >> N;
            for (int i = 0; i < refOrder(N); ++i) std::printf("%d ", refToPadded(i));
            std::printf("\n");
        } else if (cmd == "layout") {
            int B, cap, ld, gw;
            in >> B >> cap >> ld >> gw;
            const WorkLayout w{B, cap, ld, gw};
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", w.jacStride(), w.estStride(), w.offJac(), w.offEst(), w.offErr(),
                w.offMean(), w.offOut(), w.offP0(), w.offQ(), w.offGlob(), w.offVerdict(), w.doubles());
        } else if (cmd == "head" || cmd == "tables") {
            int B, ref, n;
            in >> B >> ref >> n;
            std::vector<int> idx(n > 0 ? n : 0);
            std::vector<double> w(n > 0 ? n : 0);
            for (auto& v : idx) in >> v;
            for (auto& v : w) v = readDouble(in);
            if (cmd == "head") {
                int null = 0;
                in >> null;
                std::printf("%d\n", headArgsOk(n, null == 1 ? nullptr : idx.data(), null == 2 ? nullptr : w.data(), ref, B) ? 1 : 0);
            } else {
                std::vector<double> wt(n);
                normalise(n, w.data(), wt.data());
                std::vector<Member> members;
                std::vector<int> uniq;
                buildTables(n, idx.data(), wt.data(), ref, B, members, uniq);
                for (auto& m : members) std::printf("%d %a ", m.b, m.w);
                std::printf("\n");
                for (int u : uniq) std::printf("%d ", u);
                std::printf("\n");
            }
        } else if (cmd == "ids") {
            int na, nb;
            in >> na;
            std::vector<int> a(na);
            for (auto& v : a) in >> v;
            in >> nb;
            std::vector<int> b(nb);
            for (auto& v : b) in >> v;
            std::printf("%d\n", sameIds(a.data(), na, b.data(), nb) ? 1 : 0);
        } else if (cmd == "norm") {
            int n;
            in >> n;
            std::vector<double> w(n), wt(n);
            for (auto& v : w) v = readDouble(in);
            const double ne = normalise(n, w.data(), wt.data());
            std::printf("%a\n", ne);
            for (double v : wt) std::printf("%a ", v);
            std::printf("\n");
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
