// Copy, fork and resample filters on the device (eqf_copy_filters).
//
// A copy of n filters is a gather over a pair table: pair k makes filter `dst` of the destination handle what filter `src` of the source
// handle was before the call.  The table is uploaded once and the pairs sit in a grid dimension, so the number of launches does not depend
// on n:
//   k_clone_sigma  the covariance: the source's internal extent (12 + 3 N)^2 (eqf_device.hpp: pad row / column 11 included) read with the
//                  source's leading dimension and stride, written with the destination's.  Both layouts start every row 16-byte aligned
//                  (ld is a multiple of 16 elements), so a lane moves 16 bytes per access and a wavefront one contiguous run of a row; a
//                  workgroup takes kCloneRows rows of one 256-lane column chunk and has all of its loads in flight before the first store.
//                  No arithmetic, no LDS: what is read is what is written, fp64 and fp32 alike.
//   k_clone_small  the O(N) state: Glob, p0, Q, the records of the last update and the innovation statistics, between SoA layouts of
//                  different capacity (updateOk = 0 in the destination, as eqf_set_state leaves it).
//   k_clone_restore  in the destination, what k_restore_constants does behind eqf_set_state: the pose constants and the per-landmark
//                  constants recomputed from the copied origin.
// dst == src: a source that is also somebody's destination is first copied to a staging image (the first two kernels, pairs s -> s into
// the scratch image of eqf_get_sigma_local and a small-state image of its own), and the pairs that read it are pointed there.  Filters
// that are not named are not touched.
#pragma once
#include <cstddef>

#include "eqf_device.hpp"
#include "eqf_innov.hpp"
#include "eqf_math.hpp"
#include "eqf_propagate.hpp"
#include "eqf_update.hpp"

namespace eqf {

constexpr int kCloneRows = 8;  // rows per workgroup = 16-byte loads in flight per lane

struct ClonePair {
    int dst, src;   // dst < 0: a pair the device has withdrawn (a split whose source failed); k_clone_small and k_clone_restore pass over it.
                    // k_clone_sigma does NOT: it is never handed such a table (eqf_split.hpp moves Sigma itself)
    int N;          // landmarks of the source filter: the extent moved is kLm0 + 3 N
    int fromStage;  // read the staging image instead of the source handle
};

// the small state of one handle (or of the staging image): SoA arrays with the handle's capacity
struct CloneSide {
    Glob* g;
    double *p0, *Q;                   // [B][3][cap], [B][5][cap]
    double *delta, *gamma, *gammaTot; // [B][2 cap], [B][kLm0 + 3 cap], [B][9 + 3 cap]
    double* innov;                    // [B][kInnovHead + cap] or nullptr (option off)
    int cap;
};

struct CloneSigmaArgs {
    const void* src;    // the source handle's current covariance buffer
    const void* stage;  // staging image (source layout), for pairs with fromStage
    void* dst;
    int ldSrc, ldDst;
    long long strideSrc, strideDst;
    const ClonePair* pairs;
    int nPairs;
};

// 16 bytes of T
template <typename T>
struct CloneVec;
template <>
struct CloneVec<double> {
    typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct CloneVec<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};

// grid = (ceil(max n / (256 V)), ceil(max n / kCloneRows), min(pairs, 65535)), block = 256; V = elements per 16 bytes
template <typename T>
__global__ __launch_bounds__(256) void k_clone_sigma(CloneSigmaArgs a) {
    using V = typename CloneVec<T>::type;
    constexpr int kV = int(sizeof(V) / sizeof(T));
    const int c0 = (blockIdx.x * 256 + threadIdx.x) * kV;
    const int r0 = blockIdx.y * kCloneRows;
    for (int k = blockIdx.z; k < a.nPairs; k += gridDim.z) {
        const ClonePair p = a.pairs[k];
        const int n = kLm0 + 3 * p.N;
        if (r0 >= n || c0 >= n) continue;  // (past this pair's extent: whole workgroups for all but the last chunk)
        const int rows = min(kCloneRows, n - r0);
        const T* S = static_cast<const T*>(p.fromStage ? a.stage : a.src) + (long long)p.src * a.strideSrc + (long long)r0 * a.ldSrc + c0;
        T* D = static_cast<T*>(a.dst) + (long long)p.dst * a.strideDst + (long long)r0 * a.ldDst + c0;
        if (c0 + kV <= n) {
            V v[kCloneRows];
#pragma unroll
            for (int u = 0; u < kCloneRows; ++u) v[u] = *reinterpret_cast<const V*>(S + (long long)min(u, rows - 1) * a.ldSrc);
#pragma unroll
            for (int u = 0; u < kCloneRows; ++u)
                if (u < rows) *reinterpret_cast<V*>(D + (long long)u * a.ldDst) = v[u];
        } else {  // the rows' last, partial 16 bytes: the one lane that holds them
            for (int u = 0; u < rows; ++u)
                for (int e = 0; c0 + e < n; ++e) D[(long long)u * a.ldDst + e] = S[(long long)u * a.ldSrc + e];
        }
    }
}

struct CloneSmallArgs {
    CloneSide src, stage, dst;
    int restore;    // 1: the destination is a handle (updateOk = 0, as eqf_set_state leaves it), 0: a staging image (plain copy)
    const ClonePair* pairs;
    int nPairs;
};

constexpr int kGlobWords = int(sizeof(Glob) / 8);
static_assert(sizeof(Glob) % 8 == 0 && kGlobWords <= 256 && offsetof(Glob, updateOk) % 8 == 0 && offsetof(Glob, pad_) == offsetof(Glob, updateOk) + 4,
    "k_clone_small copies Glob in 8-byte words and clears updateOk in its word");

// grid = (ceil(max(dst.cap, 1) / 256), min(pairs, 65535)), block = 256.  Beyond N the destination's p0 and Q are zeroed, as eqf_set_state
// leaves them.
__global__ __launch_bounds__(256) void k_clone_small(CloneSmallArgs a) {
    const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    const int cd = a.dst.cap;
    for (int k = blockIdx.y; k < a.nPairs; k += gridDim.y) {
        const ClonePair p = a.pairs[k];
        if (p.dst < 0) continue;  // (withdrawn on the device: eqf_split.hpp)
        const bool st = p.fromStage != 0;
        const CloneSide* sd = st ? &a.stage : &a.src;  // (uniform: scalar loads from the kernel arguments)
        const int N = p.N, cs = sd->cap;
        if (blockIdx.x == 0) {
            // Glob word by word; in a handle updateOk = 0, as eqf_set_state leaves it
            const unsigned long long* gs = reinterpret_cast<const unsigned long long*>(sd->g + p.src);
            unsigned long long* gd = reinterpret_cast<unsigned long long*>(a.dst.g + p.dst);
            if (threadIdx.x < kGlobWords) {
                unsigned long long w = gs[threadIdx.x];
                if (a.restore && threadIdx.x == int(offsetof(Glob, updateOk) / 8)) w &= 0xffffffff00000000ull;
                gd[threadIdx.x] = w;
            }
        }
        const double* sp = sd->p0 + (long long)p.src * 3 * cs;
        const double* sq = sd->Q + (long long)p.src * 5 * cs;
        double* dp = a.dst.p0 + (long long)p.dst * 3 * cd;
        double* dq = a.dst.Q + (long long)p.dst * 5 * cd;
        for (int i = tid; i < cd; i += nth) {
            const bool in = i < N;
            double P[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) P[c] = in ? sp[(long long)c * cs + i] : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[(long long)c * cd + i] = P[c];
#pragma unroll
            for (int c = 0; c < 5; ++c) dq[(long long)c * cd + i] = in ? sq[(long long)c * cs + i] : 0.0;
        }
        // the records of the last update (eqf_get_last_update)
        const double* sDelta = sd->delta + (long long)p.src * 2 * cs;
        const double* sGamma = sd->gamma + (long long)p.src * (kLm0 + 3 * cs);
        const double* sGammaTot = sd->gammaTot + (long long)p.src * (9 + 3 * cs);
        for (int i = tid; i < 2 * N; i += nth) a.dst.delta[(long long)p.dst * 2 * cd + i] = sDelta[i];
        for (int i = tid; i < kLm0 + 3 * N; i += nth) a.dst.gamma[(long long)p.dst * (kLm0 + 3 * cd) + i] = sGamma[i];
        for (int i = tid; i < 9 + 3 * N; i += nth) a.dst.gammaTot[(long long)p.dst * (9 + 3 * cd) + i] = sGammaTot[i];
        // innovation statistics: copied when both sides keep them; a destination that keeps them alone forgets its own (valid = 0)
        if (a.dst.innov) {
            const double* sInnov = sd->innov;
            for (int i = tid; i < kInnovHead + N; i += nth)
                a.dst.innov[(long long)p.dst * (kInnovHead + cd) + i] = sInnov ? sInnov[(long long)p.src * (kInnovHead + cs) + i] : 0.0;
        }
    }
}

// What k_restore_constants does behind eqf_set_state, for the destination of every pair: the per-landmark constants from the copied origin
// and, for an initialised filter, the cached pose constants -- the destination ends up with what a restore through the host leaves there.
// grid = (ceil(max(max N, 1) / 128), min(pairs, 65535)), block = 128
__global__ __launch_bounds__(128) void k_clone_restore(Glob* g, const double* p0, double* lmc, int cap, int* errflag, const ClonePair* pairs,
    int nPairs) {
    const int tid = blockIdx.x * 128 + threadIdx.x;
    for (int k = blockIdx.y; k < nPairs; k += gridDim.y) {
        const int b = pairs[k].dst, N = pairs[k].N;
        if (b < 0) continue;
        Glob& s = g[b];
        int bad = 0;
        for (int i = tid; i < N; i += gridDim.x * 128) {
            double cst[15];
            landmarkConstants(mk3(p0[((long long)b * 3 + 0) * cap + i], p0[((long long)b * 3 + 1) * cap + i], p0[((long long)b * 3 + 2) * cap + i]), cst, &bad);
            for (int c = 0; c < 15; ++c) lmc[((long long)b * 15 + c) * cap + i] = cst[c];
        }
        if (tid == 0 && s.initialised) {
            double e0[3], cd[6], ci[6];
            poseConstants(quat{s.P0q[0], s.P0q[1], s.P0q[2], s.P0q[3]}, e0, cd, ci, &bad);
            for (int i = 0; i < 3; ++i) s.eta0[i] = e0[i];
            for (int i = 0; i < 6; ++i) {
                s.cDiff[i] = cd[i];
                s.cInv[i] = ci[i];
            }
        }
        if (bad && errflag) atomicOr(errflag, 32);
    }
}

}  // namespace eqf
