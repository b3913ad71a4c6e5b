// Drives eqf_vio_amd/csrc/eqf_schmidt_host.hpp for tests/test_schmidt_host.py: one command per line on stdin, one line of integers per
// command on stdout.  Built with g++ under the address and undefined-behaviour sanitizers; no GPU, no HIP.
//   check B cap cstride nullN nullIds n[B] ids[B * cstride]      -> the code of schmidt::checkLists
//   active N nc ids[N] cids[nc]                                   -> found nA activeIdx[nA] flags[12 + 3 N]
//   own N nc ids[N] cids[nc]                                      -> gridX, entries outside c x c with exactly one owner, with another number
//                                                                    of owners, entries inside c x c with an owner, entries inside c x c
//   image B pitch { N nc ids[N] cids[nc] } x B                    -> bytes, then per filter: count, pad, activeIdx[pitch], flags[pitch]
//   bytes n nc                                                    -> 16 (n^2 - nc^2)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_schmidt_host.hpp"

namespace sc = eqf::schmidt;

static std::vector<int> readInts(std::istringstream& in, int count) {
    std::vector<int> v(static_cast<size_t>(count > 0 ? count : 0));
    for (int& x : v) in >> x;
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "check") {
            int B, cap, cstride, nullN, nullIds;
            in >> B >> cap >> cstride >> nullN >> nullIds;
            const std::vector<int> n = readInts(in, B), ids = readInts(in, B * (cstride > 0 ? cstride : 0));
            std::printf("%d\n", sc::checkLists(B, cap, nullN ? nullptr : n.data(), nullIds ? nullptr : ids.data(), cstride));
        } else if (cmd == "active" || cmd == "own") {
            int N, nc;
            in >> N >> nc;
            const std::vector<int> ids = readInts(in, N), cids = readInts(in, nc);
            std::vector<int> act;
            std::vector<unsigned char> fl;
            const int found = sc::buildActive(N, ids.data(), nc, cids.data(), act, fl);
            const int n = sc::paddedOrder(N), nA = int(act.size());
            if (cmd == "active") {
                std::printf("%d %d", found, nA);
                for (int a : act) std::printf(" %d", a);
                for (unsigned char f : fl) std::printf(" %d", int(f));
                std::printf("\n");
                continue;
            }
            // every workgroup of the launch, every entry it holds: who writes what
            std::vector<int> owners(size_t(n) * n, 0);
            const int nJT = sc::colTiles(n), grid = sc::gridX(nA, n);
            for (int t = 0; t < grid; ++t) {
                const int P = t / nJT, J = t % nJT;
                for (int r = 0; r < sc::kTile; ++r) {
                    if (sc::kTile * P + r >= nA) break;
                    const int a = act[size_t(sc::kTile * P + r)];
                    for (int c = 0; c < sc::kTile; ++c) {
                        const int j = sc::kTile * J + c;
                        if (j >= n || !sc::owns(a, j, fl.data())) continue;
                        ++owners[size_t(a) * n + j];
                        if (j != a) ++owners[size_t(j) * n + a];
                    }
                }
            }
            long long one = 0, other = 0, insideOwned = 0, inside = 0;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    const int o = owners[size_t(i) * n + j];
                    if (fl[size_t(i)] && fl[size_t(j)]) {
                        ++inside;
                        if (o) ++insideOwned;
                    } else if (o == 1) {
                        ++one;
                    } else {
                        ++other;
                    }
                }
            std::printf("%d %lld %lld %lld %lld\n", grid, one, other, insideOwned, inside);
        } else if (cmd == "image") {
            int B, pitch;
            in >> B >> pitch;
            const sc::Image im{size_t(B), size_t(pitch)};
            std::vector<char> h(im.bytes());
            for (int b = 0; b < B; ++b) {
                int N, nc;
                in >> N >> nc;
                const std::vector<int> ids = readInts(in, N), cids = readInts(in, nc);
                std::vector<int> act;
                std::vector<unsigned char> fl;
                sc::buildActive(N, ids.data(), nc, cids.data(), act, fl);
                sc::fillFilter(im, size_t(b), act, fl, h.data());
            }
            std::printf("%zu", im.bytes());
            const int* cnt = reinterpret_cast<const int*>(h.data() + im.offCount());
            const int* act = reinterpret_cast<const int*>(h.data() + im.offActive());
            const unsigned char* fl = reinterpret_cast<const unsigned char*>(h.data() + im.offFlag());
            for (int b = 0; b < B; ++b) {
                std::printf(" %d %d", cnt[2 * b], cnt[2 * b + 1]);
                for (int i = 0; i < pitch; ++i) std::printf(" %d", act[size_t(b) * pitch + i]);
                for (int i = 0; i < pitch; ++i) std::printf(" %d", int(fl[size_t(b) * pitch + i]));
            }
            std::printf("\n");
        } else if (cmd == "bytes") {
            int n, nc;
            in >> n >> nc;
            std::printf("%.0f\n", sc::countedBytes(n, nc));
        } else {
            return 2;
        }
    }
    return 0;
}
