// Driver of tests/test_workspace_host.py: eqf_workspace_host.hpp's reserve() against a counting fake backend that fails the k-th request
// (allocations and the drain count), compiled with g++ under the address and undefined-behaviour sanitizers.  Every block the backend
// hands out is a real heap block, so a piece reserve() loses shows as a leak at exit and a piece it frees twice aborts the run.
//
// stdin, one case per line:  n nCaps nCalls  { piece capIndex mapped } x n   { failAt  bytes x n } x nCalls
//   (piece 0 device, 1 pinned, 2 event; capIndex -1: the slot has no capacity of its own; failAt 0: nothing fails)
// stdout, per call one line:  ok installed nLog { code a b } x nLog   and one line with the state  { id cap mappedOk } x n  live
//   log codes: 1 / 2 / 3 allocated a device / pinned / event block (a = id, b = bytes), 4 / 5 / 6 freed one (a = id), 7 drain (a = ok),
//   8 error state cleared, 9 a request failed (a = piece)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_workspace_host.hpp"

namespace ws = eqf::workspace;

struct Fake {
    int requests = 0, failAt = 0, nextId = 1;
    std::map<void*, int> live;      // block -> id
    std::map<void*, int> kindOf;    // block -> piece
    std::vector<long long> log;
    bool fails() { return ++requests == failAt; }
    void* get(int piece, std::size_t bytes) {
        if (fails()) {
            log.insert(log.end(), {9, piece, 0});
            return nullptr;
        }
        void* p = std::malloc(2);
        live[p] = nextId++;
        kindOf[p] = piece;
        log.insert(log.end(), {1 + piece, live[p], (long long)bytes});
        return p;
    }
    void put(int piece, void* p) {
        if (!live.count(p) || kindOf[p] != piece) {
            std::fprintf(stderr, "freed a block that is not live, or through the wrong call\n");
            std::abort();
        }
        log.insert(log.end(), {4 + piece, live[p], 0});
        live.erase(p);
        std::free(p);
    }
    void* allocDevice(std::size_t bytes) { return get(0, bytes); }
    void* allocPinned(std::size_t bytes, void** mapped) {
        void* p = get(1, bytes);
        if (p && mapped) *mapped = static_cast<char*>(p) + 1;
        return p;
    }
    void* allocEvent() { return get(2, 1); }
    void freeDevice(void* p) { put(0, p); }
    void freePinned(void* p) { put(1, p); }
    void freeEvent(void* p) { put(2, p); }
    bool drain() {
        const bool ok = !fails();
        log.insert(log.end(), {7, ok ? 1 : 0, 0});
        return ok;
    }
    void clearError() { log.insert(log.end(), {8, 0, 0}); }
};

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int n = 0, nCaps = 0, nCalls = 0;
        in >> n >> nCaps >> nCalls;
        std::vector<int> piece(n), capIndex(n), isMapped(n);
        for (int i = 0; i < n; ++i) in >> piece[i] >> capIndex[i] >> isMapped[i];
        std::vector<void*> slot(n, nullptr), mapped(n, nullptr);
        std::vector<std::size_t> cap(nCaps, 0);
        Fake be;
        for (int c = 0; c < nCalls; ++c) {
            be.requests = 0;
            be.log.clear();
            in >> be.failAt;
            std::vector<ws::Want> w(n);
            for (int i = 0; i < n; ++i) {
                std::size_t bytes = 0;
                in >> bytes;
                w[i] = ws::Want{static_cast<ws::Piece>(piece[i]), &slot[i], capIndex[i] >= 0 ? &cap[capIndex[i]] : nullptr, bytes,
                    isMapped[i] ? &mapped[i] : nullptr};
            }
            const ws::Result r = ws::reserve(be, w.data(), n);
            std::cout << (r.ok ? 1 : 0) << ' ' << r.installed << ' ' << be.log.size() / 3;
            for (long long v : be.log) std::cout << ' ' << v;
            std::cout << '\n';
            for (int i = 0; i < n; ++i) {
                const bool mOk = isMapped[i] && slot[i] && mapped[i] == static_cast<char*>(slot[i]) + 1;
                std::cout << (slot[i] ? be.live.at(slot[i]) : 0) << ' ' << (capIndex[i] >= 0 ? (long long)cap[capIndex[i]] : -1) << ' ' << (mOk ? 1 : 0)
                          << ' ';
            }
            std::cout << be.live.size() << '\n';
        }
        // what the owners do when the handle goes: each slot frees what it holds -- anything else still live is reserve()'s leak
        for (int i = 0; i < n; ++i)
            if (slot[i]) be.put(piece[i], slot[i]);
    }
    return 0;
}
