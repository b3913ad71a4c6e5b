// Drives eqf_vio_amd/csrc/eqf_border_host.hpp (host only, standard library only) for tests/test_border_host.py: one case per line on stdin,
// integers on stdout.  Built with g++ under the address and undefined-behaviour sanitizers.
//   stage N            -> borderStage(N) borderOn(N) lastStages(N) blocks(eOrder(N)) rolesPlain(N) rolesBorder(N) borderRow(N, 0) (or -1)
//   omit nbMax N0 N1 ..-> bit C of omitMask as nbMax integers 0 / 1
//   const              -> kBlock kStage kRows kMaxStage
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_border_host.hpp"

using namespace eqf::border;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "stage") {
            int N;
            in >> N;
            std::printf("%d %d %d %d %d %d %d\n", borderStage(N), int(borderOn(N)), lastStages(N), blocks(eOrder(N)), rolesPlain(N), rolesBorder(N),
                borderStage(N) >= 0 ? borderRow(N, 0) : -1);
        } else if (cmd == "omit") {
            int nbMax, n;
            in >> nbMax;
            std::vector<int> counts;
            while (in >> n) counts.push_back(n);
            const unsigned long long m = omitMask(counts.data(), int(counts.size()), nbMax);
            for (int C = 0; C < nbMax; ++C) std::printf("%d ", int((m >> C) & 1ull));
            std::printf("\n");
        } else if (cmd == "const") {
            std::printf("%d %d %d %d\n", kBlock, kStage, kRows, kMaxStage);
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
