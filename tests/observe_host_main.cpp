// TEST INFRASTRUCTURE ONLY -- drives eqf_vio_amd/csrc/eqf_observe_host.hpp, compiled FOR THE HOST (g++; eqf_math.hpp only needs
// -D__HIP_PLATFORM_AMD__ and the HIP include directory for its __host__ __device__ attributes), from stdin so that
// tests/test_observe_host.py can run it under the address and undefined-behaviour sanitizers without a GPU.  Numbers travel as C99 hex
// floats (exact).  One command per line, one line of output per command:
//   entry KIND P0[3] Q[4] A CAM[7] MEAS[3]        ->  Ht[3 rows] resid[rows] notObservable     (landmarkJ, unitCam, entryRows)
//   layout B STRIDE ROWS                          ->  the offsets of SmallLayout and RowsLayout
//   head KIND CAMPF STRIDE GATE LM_GATE NULLMASK(4 bits: nk ids meas Rb)   ->  headArgsOk
//   args KIND CAMMODE(0 NULL, 1 one, 2 per filter) STRIDE B CAP LDG WANTGAMMA  NK[B] N[B] MASK[B] IDS[B STRIDE] CAM[7 | 7 B] then per
//        entry MEAS[3], R[ROWS^2]                 ->  argsCheck
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_observe_host.hpp"

namespace ob = eqf::observe;

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
            int kind;
            in >> kind;
            const auto p0 = nums(in, 3), q = nums(in, 4), a = nums(in, 1), cam = nums(in, ob::kCam), meas = nums(in, 3);
            const int rows = ob::rowsOf(kind);
            double J[9], unit[ob::kCam];
            std::vector<double> Ht(3 * rows), resid(rows);  // (exactly sized: a write past the rows is the sanitizer's to find)
            ob::landmarkJ(eqf::quat{q[0], q[1], q[2], q[3]}, a[0], J);
            ob::unitCam(cam.data(), unit);
            const int no = ob::entryRows(kind, J, eqf::mk3(p0[0], p0[1], p0[2]), unit, meas.data(), Ht.data(), resid.data());
            for (double v : Ht) std::printf("%a ", v);
            for (double v : resid) std::printf("%a ", v);
            std::printf("%d\n", no);
        } else if (cmd == "layout") {
            int B, stride, rows;
            in >> B >> stride >> rows;
            const ob::SmallLayout s{B, stride, rows};
            const ob::RowsLayout r{B, stride, rows};
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", s.offCam(), s.offMeas(), s.offR(), s.offIdx(), s.offNk(), s.offMask(), s.bytes(),
                r.offHt(), r.offResid(), r.doubles());
        } else if (cmd == "head") {
            int kind, campf, stride, nul;
            in >> kind >> campf >> stride;
            const double gate = num(in), lmGate = num(in);
            in >> nul;
            const int i = 0;
            const double d = 0.0;
            std::printf("%d\n", int(ob::headArgsOk(kind, campf, (nul & 1) ? nullptr : &i, (nul & 2) ? nullptr : &i, stride, (nul & 4) ? nullptr : &d,
                                    (nul & 8) ? nullptr : &d, gate, lmGate)));
        } else if (cmd == "args") {
            int kind, camMode, stride, B, cap, ldg, wantGamma;
            in >> kind >> camMode >> stride >> B >> cap >> ldg >> wantGamma;
            const int rows = ob::rowsOf(kind);
            const auto nk = ints(in, B), N = ints(in, B), mk = ints(in, B), ids = ints(in, size_t(B) * stride);
            std::vector<unsigned char> mask(mk.begin(), mk.end());
            const auto cam = nums(in, camMode == 2 ? size_t(B) * ob::kCam : (camMode == 1 ? ob::kCam : 0));
            // exactly sized arrays: a read past [B][stride][..] is the sanitizer's to find
            std::vector<double> meas(size_t(B) * stride * 3), R(size_t(B) * stride * rows * rows);
            for (size_t e = 0; e < size_t(B) * stride; ++e) {
                for (int i = 0; i < 3; ++i) meas[e * 3 + i] = num(in);
                for (int i = 0; i < rows * rows; ++i) R[e * rows * rows + i] = num(in);
            }
            double g = 0.0;
            std::printf("%d\n", ob::argsCheck(kind, camMode ? cam.data() : nullptr, camMode == 2, nk.data(), ids.data(), stride, meas.data(), R.data(),
                                    mask.data(), wantGamma ? &g : nullptr, ldg, B, N.data(), cap));
        } else if (!cmd.empty()) {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
