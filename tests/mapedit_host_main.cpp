// Driver of tests/test_mapedit_host.py for eqf_vio_amd/csrc/eqf_mapedit_host.hpp (host only: built with g++ and the sanitizers, no GPU, no
// HIP).  Cases arrive on stdin as whitespace-separated tokens, results leave on stdout as lines of tokens (integers; doubles as C99 hex
// floats); the expected values are computed in Python, never by this header.
// A case: `B cap rstride istride nullmask`, then per filter `nIds id..  nRemove rid[rstride]  nInsert iid[istride] p[istride][3]
// P[istride][9]`.  nullmask: 1 n_remove, 2 remove_ids, 4 n_insert, 8 insert_ids, 16 p, 32 P are handed over as NULL (their tokens are still
// read).  Every array has exactly the size the C ABI states, on the heap, so that a read or write past it is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "eqf_mapedit_host.hpp"

using namespace eqf::mapedit;

namespace {

bool token(std::string& s) { return bool(std::cin >> s); }
std::string need() {
    std::string s;
    if (!token(s)) std::exit(3);
    return s;
}
int readInt() { return std::atoi(need().c_str()); }
double readDouble() { return std::strtod(need().c_str(), nullptr); }  // (accepts "nan", "inf")

template <typename V>
void put(const V& v) {
    for (auto x : v) std::printf("%d ", int(x));
    std::printf("\n");
}

}  // namespace

int main() {
    std::string first;
    while (token(first)) {
        const int B = std::atoi(first.c_str()), cap = readInt(), rs = readInt(), is = readInt(), nullmask = readInt();
        const size_t nr = size_t(B) * size_t(rs > 0 ? rs : 0), ni = size_t(B) * size_t(is > 0 ? is : 0);
        Lists ids(B);
        std::vector<int> nRem(B), nIns(B), rid(nr), iid(ni);
        std::vector<double> p(3 * ni), P(9 * ni);
        for (int b = 0; b < B; ++b) {
            ids[b].resize(readInt());
            for (int& x : ids[b]) x = readInt();
            nRem[b] = readInt();
            for (int k = 0; k < rs; ++k) rid[size_t(b) * rs + k] = readInt();
            nIns[b] = readInt();
            for (int k = 0; k < is; ++k) iid[size_t(b) * is + k] = readInt();
            for (int k = 0; k < 3 * is; ++k) p[size_t(b) * 3 * is + k] = readDouble();
            for (int k = 0; k < 9 * is; ++k) P[size_t(b) * 9 * is + k] = readDouble();
        }
        // (an empty vector's data() may be anything: an array without entries is handed over as NULL, which the header must never read)
        Args a{};
        a.nRemove = (nullmask & 1) ? nullptr : nRem.data();
        a.removeIds = (nullmask & 2) || rid.empty() ? nullptr : rid.data();
        a.rstride = rs;
        a.nInsert = (nullmask & 4) ? nullptr : nIns.data();
        a.insertIds = (nullmask & 8) || iid.empty() ? nullptr : iid.data();
        a.istride = is;
        a.p = (nullmask & 16) || p.empty() ? nullptr : p.data();
        a.P = (nullmask & 32) || P.empty() ? nullptr : P.data();
        Plan pl;
        const int rc = plan(ids, cap, a, pl);
        std::printf("%d\n", rc);
        if (rc != kOk) continue;
        std::printf("%d %d %d %d\n", int(pl.anyRemoved), int(pl.anyInserted), pl.maxNew, pl.maxN);
        for (int b = 0; b < B; ++b) {
            put(std::vector<unsigned char>(pl.removed.begin() + size_t(b) * rs, pl.removed.begin() + size_t(b + 1) * rs));
            put(std::vector<unsigned char>(pl.inserted.begin() + size_t(b) * is, pl.inserted.begin() + size_t(b + 1) * is));
            put(pl.keep[b]);
            put(pl.accepted[b]);
            put(pl.newIds[b]);
        }
        const Image im = imageLayout(size_t(B), cap, pl);
        std::printf("%d %d %d\n", int(im.ns), int(im.withMap), int(im.bytes() <= imageCapacityBytes(size_t(B), cap)));
        std::vector<char> img(im.bytes());
        fillImage(ids, a, pl, im, img.data());
        const double* pr = reinterpret_cast<const double*>(img.data() + im.offPrior());
        const int* cnt = reinterpret_cast<const int*>(img.data() + im.offCounts());
        const int* map = reinterpret_cast<const int*>(img.data() + im.offMap());
        for (int b = 0; b < B; ++b) {
            put(std::vector<int>(cnt + 4 * b, cnt + 4 * b + 4));
            if (im.withMap) put(std::vector<int>(map + size_t(b) * cap, map + size_t(b + 1) * cap));
            for (size_t k = 0; k < im.ns * kPrior; ++k) std::printf("%a ", pr[(size_t(b) * im.ns) * kPrior + k]);
            std::printf("\n");
        }
    }
    return 0;
}
