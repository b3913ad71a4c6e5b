// Drives eqf_vio_amd/csrc/eqf_clone_host.hpp (host only, standard library only) for tests/test_clone_host.py: one case per line on stdin,
// integers on stdout.  Built with g++ under the address and undefined-behaviour sanitizers; every buffer is a std::vector of exactly the
// size the header is told about, so an index one past an end is a report, not a silent read.
//   small B cap globBytes innovHead     -> the six per-filter counts (p0 Q delta gamma gammaTot innov), then offGlob offP0 offQ offDelta
//                                          offGamma offGammaTot offInnov bytes
//   plan dstB srcB dstCap inPlace n dst[n] src[n] srcN[srcB]
//                                       -> code nMaxN nPairs nStagePairs, then "dst src N fromStage" of every pair, then of every stage pair
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_clone_host.hpp"

using namespace eqf::clone;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "small") {
            size_t B, cap, globBytes, innovHead;
            in >> B >> cap >> globBytes >> innovHead;
            const SmallLayout s{B, cap, globBytes, innovHead};
            std::printf("%zu %zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu %zu %zu %zu\n", s.p0Count(), s.qCount(), s.deltaCount(), s.gammaCount(),
                s.gammaTotCount(), s.innovCount(), s.offGlob(), s.offP0(), s.offQ(), s.offDelta(), s.offGamma(), s.offGammaTot(), s.offInnov(),
                s.bytes());
        } else if (cmd == "plan") {
            int dstB, srcB, dstCap, inPlace, n;
            in >> dstB >> srcB >> dstCap >> inPlace >> n;
            const size_t nPairs = n > 0 ? size_t(n) : 0, nSrc = srcB > 0 ? size_t(srcB) : 0;
            std::vector<int> dst(nPairs), src(nPairs), srcN(nSrc);
            for (int& v : dst) in >> v;
            for (int& v : src) in >> v;
            for (int& v : srcN) in >> v;
            // (left-overs of an earlier call: a plan starts from empty tables)
            std::vector<Pair> pairs{Pair{-7, -7, -7, -7}}, stagePairs{Pair{-7, -7, -7, -7}};
            int nMaxN = -7;
            static const int none = 0;  // (n = 0: a valid pointer that is never read)
            const int rc = plan(dstB, srcB, dstCap, inPlace != 0, n, dst.empty() ? &none : dst.data(), src.empty() ? &none : src.data(),
                srcN.data(), pairs, stagePairs, nMaxN);
            std::printf("%d %d %zu %zu", rc, nMaxN, pairs.size(), stagePairs.size());
            for (const auto* t : {&pairs, &stagePairs})
                for (const Pair& p : *t) std::printf("  %d %d %d %d", p.dst, p.src, p.N, p.fromStage);
            std::printf("\n");
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
