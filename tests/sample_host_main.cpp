// Drives eqf_vio_amd/csrc/eqf_sample_host.hpp (host only, standard library only) for tests/test_sample_host.py: one case per line on stdin, integers
// on stdout.  Built with g++ under the address and undefined-behaviour sanitizers; every buffer is a std::vector of exactly the size the
// header is told about, so an index one past an end is a report, not a silent read.
//   map first N                      -> column of every reference index (-1 below first), then the reference index of every padded index
//   grid nsamp m                     -> rowTiles paddedRows blockColumns
//   pack first N width               -> the packed row of src[i] = i + 1, then the row unpacked into a buffer of -7 (two entries beyond n)
//   fill first N                     -> the unpack with a fill value of 9
//   small B cap                      -> vecLen offScale offVec offMask (doubles) bytes, then offset and bytes of the two upload ranges
//   records B                        -> record doubles bytes, then per filter offRecord offInfo offNees(0) offNees(15)
//   draw local first nsamp z ldz eps lde stats nMax                 (z / eps / stats: 1 = given, 0 = NULL) -> 0 | 1
//   inc B ldg mask? N[B] mask[B] (bad_b bad_i kind)                 kind 0 none | 1 NaN | 2 Inf                -> 0 | 1
//   perturb first z ldz nMax B scale? (scale_b kind)                                                         -> 0 | 1
#include <cstdio>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_sample_host.hpp"

using namespace eqf::sample;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "map") {
            int first, N;
            in >> first >> N;
            const int off = cutOffset(first);
            for (int i = 0; i < refOrder(N); ++i) std::printf("%d ", i < first ? -1 : refToPadded(i) - off);
            std::printf("\n");
            for (int j = 0; j < paddedOrder(N, 0); ++j) std::printf("%d ", paddedToRef(j));
            std::printf("\n%d %d\n", off, paddedOrder(N, off < 0 ? 0 : off));
        } else if (cmd == "grid") {
            int nsamp, m;
            in >> nsamp >> m;
            std::printf("%d %d %d\n", rowTiles(nsamp), paddedRows(nsamp), blockColumns(m));
        } else if (cmd == "pack" || cmd == "fill") {
            int first, N, width = 0;
            in >> first >> N;
            if (cmd == "pack") in >> width;
            const int n = refOrder(N);
            std::vector<double> src(n), out(n + 2, -7.0);
            for (int i = 0; i < n; ++i) src[i] = i + 1;
            if (cmd == "pack") {
                std::vector<double> row(width, -3.0);
                packRow(src.data(), first, N, row.data(), width);
                for (double v : row) std::printf("%d ", int(v));
                std::printf("\n");
                unpackRow(row.data(), first, N, out.data(), nullptr);
            } else {
                std::vector<double> row(paddedOrder(N, cutOffset(first)) > 0 ? paddedOrder(N, cutOffset(first)) : 1, 5.0);
                const double nine = 9.0;
                unpackRow(row.data(), first, N, out.data(), &nine);
            }
            for (double v : out) std::printf("%d ", int(v));
            std::printf("\n");
        } else if (cmd == "small") {
            size_t B, cap;
            in >> B >> cap;
            const SmallLayout s{B, cap};
            const Range a = s.scaleRange(), v = s.vecMaskRange();
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", s.vecLen(), s.offScale(), s.offVec(), s.offMask(), s.bytes(), a.offset, a.bytes,
                v.offset, v.bytes);
        } else if (cmd == "records") {
            size_t B;
            in >> B;
            const RecordsLayout r{B};
            std::printf("%zu %zu %zu", RecordsLayout::record(), r.doubles(), r.bytes());
            for (size_t b = 0; b < B; ++b) std::printf(" %zu %zu %zu %zu", r.offRecord(b), r.offInfo(b), r.offNees(b, 0), r.offNees(b, kTileRows - 1));
            std::printf("\n");
        } else if (cmd == "draw") {
            int local, first, nsamp, hz, ldz, he, lde, hs, nMax;
            in >> local >> first >> nsamp >> hz >> ldz >> he >> lde >> hs >> nMax;
            double dummy = 0.0;
            std::printf("%d\n", int(drawArgsOk(local, first, nsamp, hz ? &dummy : nullptr, ldz, he ? &dummy : nullptr, lde, hs ? &dummy : nullptr, nMax)));
        } else if (cmd == "inc") {
            int B, ldg, hm;
            in >> B >> ldg >> hm;
            std::vector<int> N(B), m(B);
            for (int& v : N) in >> v;
            for (int& v : m) in >> v;
            int bb, bi, kind;
            in >> bb >> bi >> kind;
            std::vector<double> g(size_t(B) * (ldg > 0 ? ldg : 0), 0.25);
            std::vector<unsigned char> mask(m.begin(), m.end());
            if (kind && !g.empty()) g[size_t(bb) * ldg + bi] = kind == 1 ? std::numeric_limits<double>::quiet_NaN() : -std::numeric_limits<double>::infinity();
            // (a stride too short for a filter must be refused BEFORE an entry beyond the buffer is looked at: the vector is exactly B * ldg)
            std::printf("%d\n", int(incrementArgsOk(g.data(), ldg, hm ? mask.data() : nullptr, B, N.data())));
        } else if (cmd == "perturb") {
            int first, hz, ldz, nMax, B, hs, sb, kind;
            in >> first >> hz >> ldz >> nMax >> B >> hs >> sb >> kind;
            double dummy = 0.0;
            std::vector<double> scale(B, 0.5);
            scale[0] = 0.0;  // (a zero is a switch, not an error)
            if (kind) scale[sb] = kind == 1 ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
            std::printf("%d\n", int(perturbArgsOk(first, hz ? &dummy : nullptr, ldz, hs ? scale.data() : nullptr, B, nMax)));
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
