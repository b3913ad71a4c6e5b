// TEST INFRASTRUCTURE ONLY -- drives eqf_vio_amd/csrc/eqf_iterate_host.hpp (and eqf_observe_host.hpp under it), compiled FOR THE HOST
// (g++; eqf_math.hpp only needs -D__HIP_PLATFORM_AMD__ and the HIP include directory for its __host__ __device__ attributes), from stdin
// so that tests/test_iterate_host.py can run it under the address and undefined-behaviour sanitizers without a GPU.  Numbers travel as
// C99 hex floats (exact).  One command per line, one line of output per command:
//   args MAXLIN TOL                                ->  argsOk
//   launches STRIDE ROWS MAXLIN                    ->  extraLaunches, and the same number counted from the launch loop itself
//   layout STRIDE ROWS DREC B MAXLIN               ->  the offsets of WorkLayout, traceDoubles, offConsider, smallBytes
//   considered N LIST[N] ID                        ->  considered
//   trial KIND P0[3] Q[4] A G[3] CAM[7] MEAS[3]    ->  Ht[3 rows] r~[rows] notObservable      (trialRows)
//   run MAXLIN TOL MASKED then per solve: FAILED LASTSTEP STALLED   ->  n_lin status last_step cur   (start, afterSolve, afterRows, afterAll;
//        solves beyond the listed ones fail; the list ends the line)
//   single WORD                                    ->  n_lin status last_step   (singleReport: the call took one linearisation)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_iterate_host.hpp"

namespace it = eqf::iterate;
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

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "args") {
            int maxLin;
            in >> maxLin;
            const double tol = num(in);
            std::printf("%d\n", int(it::argsOk(maxLin, tol)));
        } else if (cmd == "launches") {
            int stride, rows, maxLin;
            in >> stride >> rows >> maxLin;
            // the launch loop as the call runs it: form, the factorisation's schedule with one right-hand-side block row, step, rows
            const int nb = it::paddedS(stride, rows) / eqf::blocks::kTile;
            int made = 0;
            for (int k = 0; k + 1 < maxLin; ++k) {
                made += 1;
                made += 1;  // diag(0)
                for (int K = 0; K < nb; ++K) {
                    const int t = nb - K - 1;
                    made += (K > 0) + (t + 1 > 0) + (t > 0);
                }
                made += 2;
            }
            if (maxLin > 1) made += 1;
            std::printf("%d %d\n", it::extraLaunches(stride, rows, maxLin), made);
        } else if (cmd == "layout") {
            int stride, rows, dRec, B, maxLin;
            in >> stride >> rows >> dRec >> B >> maxLin;
            const it::WorkLayout w{stride, rows, dRec};
            const ob::SmallLayout s{B, stride, rows};
            std::printf("%d %lld %lld %lld %lld %lld %lld %lld %lld %zu %zu %zu\n", w.mp(), w.offS(), w.offT(), w.offW(), w.offG(), w.offGn(), w.offD(),
                w.offStep(), w.strideD(), it::traceDoubles(maxLin, B, stride), it::offConsider(s), it::smallBytes(s));
        } else if (cmd == "considered") {
            int n, id;
            in >> n;
            std::vector<int> list(n);  // (exactly sized: a read past the list is the sanitizer's to find)
            for (auto& x : list) in >> x;
            in >> id;
            std::printf("%d\n", int(it::considered(list.data(), n, id)));
        } else if (cmd == "trial") {
            int kind;
            in >> kind;
            const auto p0 = nums(in, 3), q = nums(in, 4), a = nums(in, 1), g = nums(in, 3), cam = nums(in, ob::kCam), meas = nums(in, 3);
            const int rows = ob::rowsOf(kind);
            double unit[ob::kCam];
            std::vector<double> Ht(3 * rows), rt(rows);  // (exactly sized: a write past the rows is the sanitizer's to find)
            ob::unitCam(cam.data(), unit);
            const std::vector<double> Q = {q[0], q[1], q[2], q[3], a[0]};  // (the handle's [5][cap] layout with cap = 1)
            const int no = it::trialRows(kind, Q.data(), 1, 0, eqf::mk3(p0[0], p0[1], p0[2]), eqf::mk3(g[0], g[1], g[2]), unit, meas.data(),
                Ht.data(), rt.data());
            for (double v : Ht) std::printf("%a ", v);
            for (double v : rt) std::printf("%a ", v);
            std::printf("%d\n", no);
        } else if (cmd == "run") {
            int maxLin, masked;
            in >> maxLin;
            const double tol = num(in);
            in >> masked;
            it::State s = it::start();
            for (int k = 0; k + 1 < maxLin; ++k) {
                int failed = 1, stalled = 0;
                double lastStep = 0.0;
                int f;
                if (in >> f) {
                    failed = f;
                    lastStep = num(in);
                    in >> stalled;
                }
                if (masked) continue;  // (a masked filter leaves every launch at once)
                if (it::afterSolve(s, k, failed, lastStep, tol)) it::afterRows(s, k, stalled);
            }
            it::afterAll(s, maxLin, masked);
            std::printf("%d %d %a %d\n", s.nLin, s.status, s.lastStep, s.cur);
        } else if (cmd == "single") {
            int word;
            in >> word;
            const it::Report r = it::singleReport(word);
            std::printf("%d %d %a\n", r.n_lin, r.status, r.last_step);
        } else if (!cmd.empty()) {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
