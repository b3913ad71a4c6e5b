// Stand-alone driver of eqf_vio_amd/csrc/eqf_score_host.hpp for tests/test_score_host.py: built with g++ under the address and
// undefined-behaviour sanitizers, cases on stdin (one per line), results on stdout.  Floating-point values travel as hexadecimal floats.
//   check B cap ncand stride hasMask [mask x B] nb x (B ncand) ids x (B ncand stride) bearings x (B ncand stride 3)   -> code
//   match nState stateIds.. n ids..                                                                                     -> count slots.. pos..
//   option v                                                                                                            -> 0 | 1
//   plan items option B                                                                                                 -> chunk chunks counts..
//   order cap m                                                                                                         -> padded order, block columns, launches
//   work C ldW dRec                                                  -> offW offE offD offBad doubles   (all in doubles)
//   tab nItems nMatched                                              -> offRec offNisLm offY offItems offSlots bytes sizeof(Item)
//   rec nis logdet dof bad                                                                                            -> nis logdet loglik dof info
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_score_host.hpp"

namespace sc = eqf::score;

static double rd(std::istringstream& in) {
    std::string t;
    in >> t;
    return std::strtod(t.c_str(), nullptr);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "check") {
            int B, cap, ncand, stride, hasMask;
            in >> B >> cap >> ncand >> stride >> hasMask;
            const size_t items = size_t(B > 0 ? B : 0) * size_t(ncand > 0 ? ncand : 0), st = size_t(stride > 0 ? stride : 0);
            std::vector<unsigned char> mask(size_t(B > 0 ? B : 0));
            if (hasMask)
                for (auto& v : mask) {
                    int x;
                    in >> x;
                    v = (unsigned char)x;
                }
            std::vector<int> nb(items), ids(items * st);
            std::vector<double> y(items * st * 3);
            for (auto& v : nb) in >> v;
            for (auto& v : ids) in >> v;
            for (auto& v : y) v = rd(in);
            // (one element more than the tables need, so that data() is never null for an empty table)
            nb.push_back(0), ids.push_back(0), y.push_back(0.0);
            std::printf("%d\n", sc::checkArgs(B, cap, ncand, nb.data(), ids.data(), y.data(), stride, hasMask ? mask.data() : nullptr));
        } else if (cmd == "match") {
            int nState, n;
            in >> nState;
            std::vector<int> state(static_cast<size_t>(nState));
            for (auto& v : state) in >> v;
            in >> n;
            std::vector<int> ids(static_cast<size_t>(n));
            for (auto& v : ids) in >> v;
            std::vector<int> slots{-7}, pos{-7};  // (appended to, never cleared)
            const int c = sc::matchItem(nState, state.data(), n, ids.data(), slots, pos);
            std::printf("%d", c);
            if (slots.size() != size_t(c) + 1 || pos.size() != size_t(c) + 1 || slots[0] != -7 || pos[0] != -7) std::printf(" BROKEN");
            for (int k = 0; k < c; ++k) std::printf(" %d", slots[size_t(k) + 1]);
            for (int k = 0; k < c; ++k) std::printf(" %d", pos[size_t(k) + 1]);
            std::printf("\n");
        } else if (cmd == "option") {
            int v;
            in >> v;
            std::printf("%d\n", sc::chunkOptionOk(v) ? 1 : 0);
        } else if (cmd == "plan") {
            long long items;
            int option, B;
            in >> items >> option >> B;
            const int chunk = sc::chunkSize(option, B), n = sc::numChunks(items, chunk);
            std::printf("%d %d", chunk, n);
            for (int c = 0; c < n; ++c) std::printf(" %d", sc::chunkCount(items, chunk, c));
            std::printf("\n");
        } else if (cmd == "order") {
            int cap, m;
            in >> cap >> m;
            std::printf("%d %d %d\n", sc::paddedOrder(cap), sc::blockColumns(m), sc::launchesPerChunk(m));
        } else if (cmd == "work") {
            size_t C, ldW, dRec;
            in >> C >> ldW >> dRec;
            const sc::WorkLayout w{C, ldW, dRec};
            std::printf("%zu %zu %zu %zu %zu\n", w.offW(), w.offE(), w.offD(), w.offBad(), w.doubles());
        } else if (cmd == "tab") {
            size_t nItems, nMatched;
            in >> nItems >> nMatched;
            const sc::TabLayout t{nItems, nMatched};
            std::printf("%zu %zu %zu %zu %zu %zu %zu\n", t.offRec(), t.offNisLm(), t.offY(), t.offItems(), t.offSlots(), t.bytes(), sizeof(sc::Item));
        } else if (cmd == "rec") {
            const double nis = rd(in), logdet = rd(in);
            int dof, bad;
            in >> dof >> bad;
            double rec[sc::kRec];
            sc::writeRecord(rec, nis, logdet, dof, bad != 0);
            std::printf("%a %a %a %d %d %a %a %a\n", rec[0], rec[1], rec[2], int(rec[3]), int(rec[4]), rec[5], rec[6], rec[7]);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
