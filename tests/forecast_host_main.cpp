// Drives eqf_vio_amd/csrc/eqf_forecast_host.hpp (host only, standard library only) for tests/test_forecast_host.py: one case per line on
// stdin, integers on stdout.  Built with g++ under the address and undefined-behaviour sanitizers; every buffer is a std::vector of exactly
// the size the header is told about, so an index one past an end is a report, not a silent read.
//   const                       -> kMaxSteps kImuRec kLanes kBuildThreads kStepRec kHead kBaseDoubles kLmRec, then the offsets of the step
//                                  record (13), of the head (6) and of a landmark's record (6)
//   grid N B                    -> buildGrid x y threads, lmGrid x y threads
//   layout K t1 B cap           -> steps imageDoubles imageCapacityDoubles recDoubles outStride, then imageIndex(s, b) of every sample,
//                                  then outBase(b) outLm(b, 0) outLm(b, cap - 1) + kLmRec per filter, then recIndex(b, 0) recIndex(b, kMaxSteps) per filter
//   used N                      -> outUsed
//   pack K t1 B                 -> the image of samples imu[k][b][j] = 1000 k + 10 b + j + 1 and t1[b] = 7000 + b, packed
//   head f out K imu local stride                                           -> 0 | 1
//   stamps K B t1 what k b kind     what 0 none | 1 a sample's stamp | 2 a sample's rate | 3 t1[b]; kind 1 NaN | 2 Inf   -> 0 | 1
//   stride p bearing lm S ycov stride B N[B]                                 -> 0 | 1
#include <cstdio>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "eqf_forecast_host.hpp"

using namespace eqf::forecast;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "const") {
            std::printf("%d %d %d %d %d %d %d %d\n", kMaxSteps, kImuRec, kLanes, kBuildThreads, kStepRec, kHead, kBaseDoubles, kLmRec);
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", kRecStep, kRecT, kRecDt, kRecRA, kRecVC, kRecCamInv, kRecOC, kRecVCcur, kRecSb,
                kRecFg, kRecFv, kRecNb, kRecNb + 15);
            std::printf("%d %d %d %d %d %d\n", kHeadTime, kHeadSteps, kHeadFlag, kHeadPoseQ, kHeadPoseX, kHeadVel);
            std::printf("%d %d %d %d %d %d\n", kLmP, kLmBearing, kLmCov, kLmS, kLmYcov, kLmFlag);
        } else if (cmd == "grid") {
            int N, B;
            in >> N >> B;
            const Grid a = buildGrid(B), b = lmGrid(N, B);
            std::printf("%d %d %d %d %d %d\n", a.x, a.y, a.threads, b.x, b.y, b.threads);
        } else if (cmd == "layout") {
            int K, t1, B, cap;
            in >> K >> t1 >> B >> cap;
            std::printf("%d %zu %zu %zu %zu\n", steps(K, t1 != 0), imageDoubles(K, t1 != 0, B), imageCapacityDoubles(B), recDoubles(B), outStride(cap));
            for (int s = 0; s < steps(K, t1 != 0); ++s)
                for (int b = 0; b < B; ++b) std::printf("%zu ", imageIndex(s, b, B));
            std::printf("\n");
            for (int b = 0; b < B; ++b) std::printf("%zu %zu %zu ", outBase(cap, b), outLm(cap, b, 0), outLm(cap, b, cap - 1) + kLmRec);
            std::printf("\n");
            for (int b = 0; b < B; ++b) std::printf("%zu %zu ", recIndex(b, 0), recIndex(b, kMaxSteps));
            std::printf("\n");
        } else if (cmd == "used") {
            int N;
            in >> N;
            std::printf("%zu\n", outUsed(N));
        } else if (cmd == "pack") {
            int K, t1, B;
            in >> K >> t1 >> B;
            std::vector<double> imu(size_t(K) * B * 7), t(B), img(imageDoubles(K, t1 != 0, B), -3.0);
            for (int k = 0; k < K; ++k)
                for (int b = 0; b < B; ++b)
                    for (int j = 0; j < 7; ++j) imu[(size_t(k) * B + b) * 7 + j] = 1000 * k + 10 * b + j + 1;
            for (int b = 0; b < B; ++b) t[b] = 7000 + b;
            for (int k = 0; k < K; ++k)
                for (int b = 0; b < B; ++b) packSample(imu.data() + (size_t(k) * B + b) * 7, img.data() + imageIndex(k, b, B));
            if (t1)
                for (int b = 0; b < B; ++b) packStamp(t[b], img.data() + imageIndex(K, b, B));
            for (double v : img) std::printf("%d ", int(v));
            std::printf("\n");
        } else if (cmd == "head") {
            int hf, ho, K, hi, local, stride;
            in >> hf >> ho >> K >> hi >> local >> stride;
            double dummy = 0.0;
            std::printf("%d\n", int(headArgsOk(hf ? &dummy : nullptr, ho ? &dummy : nullptr, K, hi ? &dummy : nullptr, local, stride)));
        } else if (cmd == "stamps") {
            int K, B, ht, what, k, b, kind;
            in >> K >> B >> ht >> what >> k >> b >> kind;
            std::vector<double> imu(size_t(K) * B * 7, 0.5), t(B, 0.25);
            const double bad = kind == 1 ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
            if (what == 1) imu[(size_t(k) * B + b) * 7] = bad;
            if (what == 2) imu[(size_t(k) * B + b) * 7 + 3] = bad;
            if (what == 3) t[b] = bad;
            std::printf("%d\n", int(stampsOk(K, K ? imu.data() : nullptr, ht ? t.data() : nullptr, B)));
        } else if (cmd == "stride") {
            int p, be, lm, S, yc, stride, B;
            in >> p >> be >> lm >> S >> yc >> stride >> B;
            std::vector<int> N(B);
            for (int& v : N) in >> v;
            const Wants w{p != 0, be != 0, lm != 0, S != 0, yc != 0};
            std::printf("%d\n", int(strideOk(w, stride, B, N.data())));
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
