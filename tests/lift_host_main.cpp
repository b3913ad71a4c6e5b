// Drives eqf_vio_amd/csrc/eqf_lift_host.hpp (host only, standard library only) for tests/test_lift_host.py: one case per line on stdin, integers
// on stdout.  Built with g++ under the address and undefined-behaviour sanitizers; every buffer is a std::vector of exactly the size the
// header is told about, so an index one past an end is a report, not a silent read.
//   kind option useLift useDiscrete N nMax  -> optionOk callKind filterKind callFactors
//   shape N nMax                            -> order(N) rhsPitch(nMax) blockColumns(nMax) rhsGroups(nMax) rhsColumn(N - 1, 2)
//   pack N extra                            -> the kRhs rows (pitch order(N) + extra, filled with -9) packed from Z[(3 i + r) * 6 + c] =
//                                              100 (3 i + r) + c + 1 and gl[j] = -(j + 1), row by row
//   report kind info                        -> the record {kind, info, 1 .. 6, 7, 8} unpacked: kind info 1 2 3 4 5 6 7 8
//   merge word                              -> mergeInfo(word) updateSolved(word)
//   update word dof hasIdle                 -> updateReport of the record {10.5, -2.25, 3.125, word, -7 ...}: nis logdet_S loglik (hex floats)
//                                              dof info
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_lift_host.hpp"

using namespace eqf::lift;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "kind") {
            int option, useLift, useDiscrete, N, nMax;
            in >> option >> useLift >> useDiscrete >> N >> nMax;
            const int k = callKind(option, useLift, useDiscrete);
            std::printf("%d %d %d %d\n", int(optionOk(option)), k, filterKind(k, N), int(callFactors(k, nMax)));
        } else if (cmd == "shape") {
            int N, nMax;
            in >> N >> nMax;
            std::printf("%d %d %d %d %d\n", order(N), rhsPitch(nMax), blockColumns(nMax), rhsGroups(nMax), N > 0 ? rhsColumn(N - 1, 2) : -1);
        } else if (cmd == "pack") {
            int N, extra;
            in >> N >> extra;
            const int ldE = order(N) + extra;
            std::vector<double> Z(size_t(3 * N) * 6), gl(size_t(3 * N)), E(size_t(kRhs) * ldE, -9.0);
            for (int j = 0; j < 3 * N; ++j) {
                for (int c = 0; c < 6; ++c) Z[size_t(j) * 6 + c] = 100.0 * j + c + 1;
                gl[j] = -(j + 1.0);
            }
            packRhs(Z.data(), gl.data(), N, E.data(), ldE);
            for (int r = 0; r < kRhs; ++r) {
                for (int j = 0; j < ldE; ++j) std::printf("%d ", int(E[size_t(r) * ldE + j]));
                std::printf("\n");
            }
        } else if (cmd == "report") {
            int kind, info;
            in >> kind >> info;
            std::vector<double> rec(kRec, 0.0);
            rec[0] = kind;
            rec[1] = info;
            for (int i = 0; i < 8; ++i) rec[2 + i] = i + 1.0;
            Report r;
            unpackReport(rec.data(), &r);
            std::printf("%d %d ", r.kind, r.info);
            for (double v : r.DeltaU) std::printf("%d ", int(v));
            std::printf("%d %d\n", int(r.min_pivot), int(r.pivot_ratio));
        } else if (cmd == "merge") {
            int word;
            in >> word;
            std::printf("%d %d\n", mergeInfo(word), int(updateSolved(word)));
        } else if (cmd == "update") {
            int word, dof, hasIdle;
            in >> word >> dof >> hasIdle;
            std::vector<double> rec(kHead, -7.0);  // (exactly one record: nis 10.5, logdet_S -2.25, loglik 3.125, the verdict word)
            rec[0] = 10.5;
            rec[1] = -2.25;
            rec[2] = 3.125;
            rec[3] = word;
            const UpdateReport r = updateReport(rec.data(), dof, hasIdle != 0);
            std::printf("%a %a %a %d %d\n", r.nis, r.logdet_S, r.loglik, r.dof, r.info);
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
