// TEST INFRASTRUCTURE ONLY -- drives eqf_vio_amd/csrc/eqf_blocks_host.hpp (host only, standard library only) from stdin so that
// tests/test_blocks_host.py can run it under the address and undefined-behaviour sanitizers without a GPU.  Numbers travel as C99 hex
// floats (exact).  One command per line, one line of output per command:
//   entry ROWS LOCAL LM_GATE IDX  H[3 ROWS] J[9] SII[9] R[ROWS^2] RESID[ROWS]  ->  Ht[3 ROWS] d2 verdict
//   compact NK USED[NK]                                                        ->  count pos[NK] ent[count]
//   layout B STRIDE ROWS LD DREC                                               ->  the offsets of SmallLayout and WorkLayout
//   grid N STRIDE                                                              ->  rowTiles triTiles rhsBlocks pairTiles
//   head LOCAL ROWS STRIDE GATE LM_GATE NULLMASK(5 bits: nk ids Hb resid Rb)    ->  headArgsOk
//   args ROWS STRIDE B CAP LDG WANTGAMMA  NK[B] N[B] MASK[B] IDS[B STRIDE] then per entry H, RESID, R as above  ->  argsCheck
//   find N ID IDS[N]                                                           ->  findId
//   gamma N ZERO SRC[12 + 3 N]                                                  ->  unpackGamma
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_blocks_host.hpp"

namespace bl = eqf::blocks;

static double num(std::istringstream& in) {
    std::string t;
    in >> t;
    return std::strtod(t.c_str(), nullptr);
}
static std::vector<double> nums(std::istringstream& in, size_t n) {
    std::vector<double> v(n);
    for (auto& x : v) x = num(in);
    return v;
}
static std::vector<int> ints(std::istringstream& in, size_t n) {
    std::vector<int> v(n);
    for (auto& x : v) in >> x;
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "entry") {
            int rows, local, idx;
            in >> rows >> local;
            const double lmGate = num(in);
            in >> idx;
            const auto H = nums(in, 3 * rows), J = nums(in, 9), Sii = nums(in, 9), R = nums(in, size_t(rows) * rows), r = nums(in, rows);
            std::vector<double> Ht(3 * rows), S(9, 0.0);
            bl::formRows(rows, H.data(), local ? J.data() : nullptr, Ht.data());
            bl::entryS(rows, Ht.data(), Sii.data(), R.data(), S.data());
            const double d2 = bl::entryD2(rows, S.data(), r.data());
            for (double v : Ht) std::printf("%a ", v);
            std::printf("%a %d\n", d2, bl::entryVerdict(idx, d2, lmGate));
        } else if (cmd == "compact") {
            int nk;
            in >> nk;
            const auto used = ints(in, nk);
            std::vector<int> pos(nk), ent(nk);
            const int cnt = bl::compact(nk, used.data(), pos.data(), ent.data());
            std::printf("%d", cnt);
            for (int k = 0; k < nk; ++k) std::printf(" %d", pos[k]);
            for (int p = 0; p < cnt; ++p) std::printf(" %d", ent[p]);
            std::printf("\n");
        } else if (cmd == "layout") {
            int B, stride, rows, ld, drec;
            in >> B >> stride >> rows >> ld >> drec;
            const bl::SmallLayout s{B, stride, rows};
            const bl::WorkLayout w{ld, stride, rows, drec};
            std::printf("%zu %zu %zu %zu %zu %zu %zu %d %d %lld %lld %lld %lld %lld %d %d %d %d %d %d\n", s.offH(), s.offResid(), s.offR(), s.offIdx(),
                s.offNk(), s.offMask(), s.bytes(), w.mp(), w.nb(), w.offM(), w.offHt(), w.offGamma(), w.offD(), w.strideD(), w.offUsed(),
                w.offPos(), w.offEnt(), w.offCount(), w.offBad(), w.strideI());
        } else if (cmd == "grid") {
            int N, stride;
            in >> N >> stride;
            std::printf("%d %d %d %d\n", bl::rowTiles(N), bl::triTiles(bl::rowTiles(N)), bl::rhsBlocks(bl::paddedOrder(N)), bl::pairTiles(stride));
        } else if (cmd == "head") {
            int local, rows, stride, nul;
            in >> local >> rows >> stride;
            const double gate = num(in), lmGate = num(in);
            in >> nul;
            const int i = 0;
            const double d = 0.0;
            std::printf("%d\n", int(bl::headArgsOk(local, rows, (nul & 1) ? nullptr : &i, (nul & 2) ? nullptr : &i, stride, (nul & 4) ? nullptr : &d,
                                    (nul & 8) ? nullptr : &d, (nul & 16) ? nullptr : &d, gate, lmGate)));
        } else if (cmd == "args") {
            int rows, stride, B, cap, ldg, wantGamma;
            in >> rows >> stride >> B >> cap >> ldg >> wantGamma;
            const auto nk = ints(in, B), N = ints(in, B), mk = ints(in, B), ids = ints(in, size_t(B) * stride);
            std::vector<unsigned char> mask(mk.begin(), mk.end());
            // exactly sized arrays: a read past [B][stride][..] is the sanitizer's to find
            std::vector<double> H(size_t(B) * stride * rows * 3), r(size_t(B) * stride * rows), R(size_t(B) * stride * rows * rows);
            for (size_t e = 0; e < size_t(B) * stride; ++e) {
                for (int i = 0; i < 3 * rows; ++i) H[e * rows * 3 + i] = num(in);
                for (int i = 0; i < rows; ++i) r[e * rows + i] = num(in);
                for (int i = 0; i < rows * rows; ++i) R[e * rows * rows + i] = num(in);
            }
            double g = 0.0;
            std::printf("%d\n", bl::argsCheck(rows, nk.data(), ids.data(), stride, H.data(), r.data(), R.data(), mask.data(), wantGamma ? &g : nullptr,
                                    ldg, B, N.data(), cap));
        } else if (cmd == "find") {
            int N, id;
            in >> N >> id;
            const auto ids = ints(in, N);
            std::printf("%d\n", bl::findId(ids.data(), N, id));
        } else if (cmd == "gamma") {
            int N, zero;
            in >> N >> zero;
            const auto src = nums(in, bl::paddedOrder(N));
            std::vector<double> dst(bl::refOrder(N));
            bl::unpackGamma(src.data(), N, dst.data(), zero);
            for (double v : dst) std::printf("%a ", v);
            std::printf("\n");
        } else if (!cmd.empty()) {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
