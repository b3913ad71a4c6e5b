// Drives eqf_vio_amd/csrc/eqf_split_host.hpp (host only, standard library only) for tests/test_split_host.py: one case per line on stdin, integers
// on stdout.  Built with g++ under the address and undefined-behaviour sanitizers; every buffer is a std::vector of exactly the size the
// header is told about, so an index one past an end is a report, not a silent read.
//   head B local a n dst[n] src[n] (bad_k kind what)      a: 1 = given, 0 = NULL; n < 0 is passed on as it is; kind 0 none | 1 NaN | 2 Inf |
//                                                        3 the value -0.25 | 4 the value 1.5; what 0 shift | 1 shrink | 2 NULL dst_idx |
//                                                        3 NULL src_idx | 4 NULL shift | 5 NULL shrink                       -> return code
//   row B lda ldg n src[n] N[B] (bad_b bad_i kind)        ldg < 0: no gamma; entry bad_i of filter bad_b's row is NaN (1) or Inf (2)
//                                                                                                                              -> return code
//   group B n dst[n] src[n] N[B]                         -> ns np maxN, then per source "src N first count", then per child
//                                                           "dst pair call source", then per pair "dst src N fromStage"
//   image B cap n dst[n] src[n] N[B]                     rows a[b][i] = 1000 b + i + 1, shift[k] = k + 1, shrink[k] = 1 / (k + 2): fills an
//                                                        image of exactly Image::bytes() -> bytes ldr, then per source its row (ldr
//                                                        integers), then shift and 1 / shrink in the child table's order
//   grid maxN                                            -> axisBlocks tileRowBlocks tileColBlocks paddedOrder
#include <cstdio>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_split_host.hpp"

using namespace eqf::split;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "head") {
            int B, local, ga, n, badK, kind, what;
            in >> B >> local >> ga >> n;
            const int m = n > 0 ? n : 0;
            std::vector<int> dst(m), src(m);
            for (int& v : dst) in >> v;
            for (int& v : src) in >> v;
            in >> badK >> kind >> what;
            std::vector<double> a(1, 0.0), shift(m, 0.5), shrink(m, 0.25);
            const double vals[] = {0.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -0.25, 1.5};
            if (kind > 0 && what == 0) shift[badK] = vals[kind];
            if (kind > 0 && what == 1) shrink[badK] = vals[kind];
            std::printf("%d\n", headCheck(B, local, ga ? a.data() : nullptr, n, what == 2 ? nullptr : dst.data(), what == 3 ? nullptr : src.data(),
                                    what == 4 ? nullptr : shift.data(), what == 5 ? nullptr : shrink.data()));
        } else if (cmd == "row") {
            int B, lda, ldg, n, badB, badI, kind;
            in >> B >> lda >> ldg >> n;
            std::vector<int> src(n), N(B);
            for (int& v : src) in >> v;
            for (int& v : N) in >> v;
            in >> badB >> badI >> kind;
            std::vector<double> a(size_t(B) * size_t(lda), 1.0);
            if (kind == 1) a[size_t(badB) * lda + badI] = std::numeric_limits<double>::quiet_NaN();
            if (kind == 2) a[size_t(badB) * lda + badI] = -std::numeric_limits<double>::infinity();
            std::printf("%d\n", rowCheck(a.data(), lda, n, src.data(), ldg, N.data()));
        } else if (cmd == "group" || cmd == "image") {
            int B, cap = 0, n;
            in >> B;
            if (cmd == "image") in >> cap;
            in >> n;
            std::vector<int> dst(n), src(n), N(B);
            for (int& v : dst) in >> v;
            for (int& v : src) in >> v;
            for (int& v : N) in >> v;
            Plan p;
            group(B, n, dst.data(), src.data(), N.data(), p);
            if (cmd == "group") {
                std::printf("%d %d %d\n", int(p.sources.size()), int(p.pairs.size()), p.maxN);
                for (const auto& s : p.sources) std::printf("%d %d %d %d\n", s.src, s.N, s.first, s.count);
                for (const auto& c : p.children) std::printf("%d %d %d %d\n", c.dst, c.pair, c.call, c.source);
                for (const auto& q : p.pairs) std::printf("%d %d %d %d\n", q.dst, q.src, q.N, q.fromStage);
                continue;
            }
            const Image im{size_t(B), size_t(cap)};
            const int lda = refOrder(cap) + 3;
            std::vector<double> a(size_t(B) * lda), shift(n), shrink(n);
            for (int b = 0; b < B; ++b)
                for (int i = 0; i < lda; ++i) a[size_t(b) * lda + i] = 1000.0 * b + i + 1;
            for (int k = 0; k < n; ++k) {
                shift[k] = k + 1;
                shrink[k] = 1.0 / (k + 2);
            }
            std::vector<char> img(im.bytes(), char(0x5a));
            fillImage(im, p, a.data(), lda, shift.data(), shrink.data(), img.data());
            std::printf("%d %d\n", int(im.bytes()), int(im.ldr()));
            const double* rows = reinterpret_cast<const double*>(img.data() + im.offRows());
            for (size_t i = 0; i < p.sources.size(); ++i) {
                for (size_t j = 0; j < im.ldr(); ++j) std::printf("%d ", int(rows[i * im.ldr() + j]));
                std::printf("\n");
            }
            const double* sh = reinterpret_cast<const double*>(img.data() + im.offShift());
            const double* sk = reinterpret_cast<const double*>(img.data() + im.offShrink());
            for (int k = 0; k < n; ++k) std::printf("%d ", int(sh[k]));
            std::printf("\n");
            for (int k = 0; k < n; ++k) std::printf("%d ", int(1.0 / sk[k] + 0.5));
            std::printf("\n");
            // the tables are the plan's, byte for byte
            const Source* ss = reinterpret_cast<const Source*>(img.data() + im.offSources());
            const Child* cs = reinterpret_cast<const Child*>(img.data() + im.offChildren());
            const Pair* ps = reinterpret_cast<const Pair*>(img.data() + im.offPairs());
            int same = 1;
            for (size_t i = 0; i < p.sources.size(); ++i) same &= ss[i].src == p.sources[i].src && ss[i].first == p.sources[i].first;
            for (size_t i = 0; i < p.children.size(); ++i) same &= cs[i].dst == p.children[i].dst && cs[i].pair == p.children[i].pair;
            for (size_t i = 0; i < p.pairs.size(); ++i) same &= ps[i].dst == p.pairs[i].dst && ps[i].src == p.pairs[i].src && ps[i].N == p.pairs[i].N;
            std::printf("%d\n", same);
        } else if (cmd == "grid") {
            int maxN;
            in >> maxN;
            std::printf("%d %d %d %d\n", axisBlocks(maxN), tileRowBlocks(maxN), tileColBlocks(maxN), paddedOrder(maxN));
        }
    }
    return 0;
}
