// Driver of tests/test_lie_exact.py for eqf_vio_amd/csrc/eqf_math.hpp compiled FOR THE HOST (g++ with the sanitizers, no GPU; the header
// only needs -D__HIP_PLATFORM_AMD__ and the HIP include directory for its __host__ __device__ attributes).  One case per line on stdin,
// `name` followed by doubles; one line of doubles (%.17g) per case on stdout, the `bad` flag of the function last where it has one.  The
// expected values are computed in Python with mpmath (tests/lie_exact.py), never by this header.
//   expc t                       -> A B C                         expCoefficients
//   se3exp w(3) v(3)             -> q(4) x(3)                     se3Exp
//   so3exp w(3)                  -> q(4)                          so3Exp
//   so3fv origin(3) dest(3)      -> q(4) bad                      so3FromVectors
//   srot pole(3)                 -> q(4) bad                      sphereRotQ
//   rotm o(3) d(3)               -> R(9) bad                      rotFromUnitVectors (UNIT inputs)
//   cdiff eta(3) pole(3)         -> D(6) bad                      stereoChartDiff
//   cinv pole(3)                 -> D(6) bad                      stereoChartInvDiffAtZero
//   chart eta(3) pole(3)         -> y(2) bad                      stereoChart
//   m2q q(4)                     -> q(4)                          m2q(q2m(q))
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "eqf_math.hpp"

using namespace eqf;

namespace {

bool token(std::string& s) { return static_cast<bool>(std::cin >> s); }
double readDouble() {
    std::string s;
    if (!token(s)) std::exit(3);
    return std::strtod(s.c_str(), nullptr);
}
d3 read3() {
    const double x = readDouble(), y = readDouble(), z = readDouble();
    return mk3(x, y, z);
}
void put(const double* v, int n) {
    for (int i = 0; i < n; ++i) std::printf("%.17g ", v[i]);
}
void putq(quat q) {
    const double v[4] = {q.w, q.x, q.y, q.z};
    put(v, 4);
}
void endl(int bad = -1) {
    if (bad >= 0) std::printf("%d", bad);
    std::printf("\n");
}

}  // namespace

int main() {
    std::string name;
    while (token(name)) {
        int bad = 0;
        if (name == "expc") {
            double v[3];
            expCoefficients(readDouble(), &v[0], &v[1], &v[2]);
            put(v, 3);
            endl();
        } else if (name == "se3exp") {
            const d3 w = read3(), v = read3();
            const se3 T = se3Exp(w, v);
            putq(T.q);
            const double x[3] = {T.x.x, T.x.y, T.x.z};
            put(x, 3);
            endl();
        } else if (name == "so3exp") {
            putq(so3Exp(read3()));
            endl();
        } else if (name == "so3fv") {
            const d3 o = read3(), d = read3();
            putq(so3FromVectors(o, d, &bad));
            endl(bad);
        } else if (name == "srot") {
            putq(sphereRotQ(read3(), &bad));
            endl(bad);
        } else if (name == "rotm") {
            const d3 o = read3(), d = read3();
            const m33 R = rotFromUnitVectors(o, d, &bad);
            put(R.a, 9);
            endl(bad);
        } else if (name == "cdiff") {
            const d3 eta = read3(), pole = read3();
            double D[6];
            stereoChartDiff(eta, pole, D, &bad);
            put(D, 6);
            endl(bad);
        } else if (name == "cinv") {
            double D[6];
            stereoChartInvDiffAtZero(read3(), D, &bad);
            put(D, 6);
            endl(bad);
        } else if (name == "chart") {
            const d3 eta = read3(), pole = read3();
            double y[2];
            stereoChart(eta, pole, &y[0], &y[1], &bad);
            put(y, 2);
            endl(bad);
        } else if (name == "m2q") {
            const double w = readDouble(), x = readDouble(), y = readDouble(), z = readDouble();
            putq(m2q(q2m(quat{w, x, y, z})));
            endl();
        } else {
            std::fprintf(stderr, "unknown case %s\n", name.c_str());
            return 2;
        }
    }
    return 0;
}
