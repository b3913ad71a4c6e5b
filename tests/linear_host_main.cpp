// Drives eqf_vio_amd/csrc/eqf_linear_host.hpp (host only, standard library only) for tests/test_linear_host.py: one case per line on stdin,
// integers on stdout.  Built with g++ under the address and undefined-behaviour sanitizers; every buffer is a std::vector of exactly the
// size the header is told about, so an index one past an end is a report, not a silent read.
//   map N                            -> padded index of every reference index, then the reference index of every padded index
//   grid N                           -> refOrder paddedOrder rowTiles triTiles, then "I J" of every tile of the lower triangle in launch order
//   layout B cap ld                  -> SmallLayout offH offResid offR offMask bytes, WorkLayout offHt offBt offY offGamma stride
//   pack m N ldh ldr                 -> 16 rows of H[k][i] = 100 (k + 1) + i + 1 packed (ldr entries each), then resid (16), then R (16 x 16)
//                                       of R[k][l] = 10 (k + 1) + l + 1
//   gamma N zero                     -> gamma unpacked from src[j] = j + 1 into a buffer of -7 (two entries beyond n)
//   head local m H resid R gate_kind                                 gate_kind 0: 9.0 | 1: +inf | 2: NaN | 3: 0 | 4: -1    -> 0 | 1
//   args m B ldh gamma? ldg mask? N[B] mask[B] what b k i kind       what 0 none | 1 H | 2 resid | 3 R (row k, column i); kind 1 NaN | 2 Inf -> 0 | 1
#include <cstdio>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_linear_host.hpp"

using namespace eqf::linear;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "map") {
            int N;
            in >> N;
            for (int i = 0; i < refOrder(N); ++i) std::printf("%d ", refToPadded(i));
            std::printf("\n");
            for (int j = 0; j < paddedOrder(N); ++j) std::printf("%d ", paddedToRef(j));
            std::printf("\n");
        } else if (cmd == "grid") {
            int N;
            in >> N;
            const int nt = rowTiles(N);
            std::printf("%d %d %d %d\n", refOrder(N), paddedOrder(N), nt, triTiles(nt));
            for (int t = 0; t < triTiles(nt); ++t) {
                int I, J;
                triTile(t, &I, &J);
                std::printf("%d %d ", I, J);
            }
            std::printf("\n");
        } else if (cmd == "layout") {
            int B, cap, ld;
            in >> B >> cap >> ld;
            const SmallLayout s{B, refOrder(cap)};
            const WorkLayout w{ld};
            std::printf("%zu %zu %zu %zu %zu %lld %lld %lld %lld %lld\n", s.offH(), s.offResid(), s.offR(), s.offMask(), s.bytes(), w.offHt(),
                w.offBt(), w.offY(), w.offGamma(), w.stride());
        } else if (cmd == "pack") {
            int m, N, ldh, ldr;
            in >> m >> N >> ldh >> ldr;
            std::vector<double> H(size_t(m) * ldh, -1.0), r(m), R(size_t(m) * m);
            for (int k = 0; k < m; ++k) {
                for (int i = 0; i < refOrder(N); ++i) H[size_t(k) * ldh + i] = 100 * (k + 1) + i + 1;
                r[k] = k + 1;
                for (int l = 0; l < m; ++l) R[size_t(k) * m + l] = 10 * (k + 1) + l + 1;
            }
            std::vector<double> dH(size_t(kRows) * ldr, -3.0), dr(kRows, -3.0), dR(kRows * kRows, -3.0);
            packFilter(m, N, H.data(), ldh, r.data(), R.data(), dH.data(), ldr, dr.data(), dR.data());
            for (const auto* v : {&dH, &dr, &dR}) {
                for (double x : *v) std::printf("%d ", int(x));
                std::printf("\n");
            }
        } else if (cmd == "gamma") {
            int N, zero;
            in >> N >> zero;
            std::vector<double> src(paddedOrder(N)), out(refOrder(N) + 2, -7.0);
            for (size_t j = 0; j < src.size(); ++j) src[j] = double(j + 1);
            unpackGamma(src.data(), N, out.data(), zero);
            for (double v : out) std::printf("%d ", int(v));
            std::printf("\n");
        } else if (cmd == "head") {
            int local, m, hH, hr, hR, gk;
            in >> local >> m >> hH >> hr >> hR >> gk;
            const double gates[5] = {9.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(), 0.0, -1.0};
            double dummy = 0.0;
            std::printf("%d\n", int(headArgsOk(local, m, hH ? &dummy : nullptr, hr ? &dummy : nullptr, hR ? &dummy : nullptr, gates[gk])));
        } else if (cmd == "args") {
            int m, B, ldh, hg, ldg, hm;
            in >> m >> B >> ldh >> hg >> ldg >> hm;
            std::vector<int> N(B), mk(B);
            for (int& v : N) in >> v;
            for (int& v : mk) in >> v;
            int what, b, k, i, kind;
            in >> what >> b >> k >> i >> kind;
            const int mm = m > 0 ? m : 0, lh = ldh > 0 ? ldh : 0;
            std::vector<double> H(size_t(B) * mm * lh, 0.5), r(size_t(B) * mm, 0.25), R(size_t(B) * mm * mm, 2.0), g(size_t(B) * (ldg > 0 ? ldg : 0));
            std::vector<unsigned char> mask(mk.begin(), mk.end());
            const double bad = kind == 1 ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
            if (what == 1) H[(size_t(b) * m + k) * ldh + i] = bad;
            if (what == 2) r[size_t(b) * m + k] = bad;
            if (what == 3) R[(size_t(b) * m + k) * m + i] = bad;
            // (a stride too short for a filter must be refused BEFORE an entry beyond the buffers is looked at: they are exactly B * m * ldh ..)
            std::printf("%d\n", int(argsOk(m, H.data(), ldh, r.data(), R.data(), hm ? mask.data() : nullptr, hg ? g.data() : nullptr, ldg, B, N.data())));
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
