// Explicit landmark removal and insertion with priors (eqf_edit_landmarks; gfx950).
//
// Device side of VIOFilter::removeLandmarkAtIndex / addNewLandmarks (eqf_vio/src/VIOFilter.cpp:345-427) for ids, positions and covariances
// of the CALLER's choosing.  Who goes, who comes and in which order is decided on the host (eqf_mapedit_host.hpp, which also lays out the
// image read here); the kernels move Sigma and the per-landmark arrays.  Two launches, one per call:
//   k_mapedit_move    some filter loses a landmark: every filter's Sigma goes into the other buffer through its keep map (the ping-pong
//                     parity is shared by the batch; a filter without an edit passes the identity), new rows and columns are written on the way
//   k_mapedit_append  nobody loses anything: only the new rows, columns and blocks are written, in place, O(n * new)
// No atomics on values, no list in LDS (the map is read from global memory, where the whole launch shares it in L2): no bound on N.
#pragma once
#include "eqf_churn.hpp"

namespace eqf {

constexpr int kMapPrior = 12;  // doubles per accepted insertion: p (3), P mirrored (3 x 3); mapedit::kPrior

struct MapEditArgs {
    Glob* g;
    const double* prior;  // [B][ns][kMapPrior]
    const int* cnt;       // [B][4]: kept, new, old count
    const int* map;       // [B][cap] old index of kept landmark j (k_mapedit_move only)
    int ns, cap;
    double *p0, *Q, *lmc, *scratch;
    int* errflag;
    const void* Sin;      // k_mapedit_move: the current buffer
    void* Sout;           // k_mapedit_move: the other one; k_mapedit_append: the current one
    long long sigmaStride;
    int ld;
};

// Entry (R, Cc) of the grown Sigma where R or Cc belongs to a new landmark (nvK = kLm0 + 3 * kept): the landmark's own prior block, else 0.
template <typename T>
__device__ __forceinline__ T mapeditNewEntry(const double* prior, int nvK, int R, int Cc) {
    const int lo = min(R, Cc);
    if (lo < nvK) return (T)0;
    const int lr = (R - nvK) / 3, lc = (Cc - nvK) / 3;
    if (lr != lc) return (T)0;
    return (T)prior[(long long)lr * kMapPrior + 3 + 3 * ((R - nvK) % 3) + (Cc - nvK) % 3];
}

// The new landmarks of filter b behind its nK kept ones, by the threads of ONE workgroup: p0 = p as uploaded, Q = identity, the constants
// from the origin landmark AS STORED (see k_append: a restored filter recomputes them from p0 and has to continue bitwise).
__device__ __forceinline__ void mapeditWriteNew(const MapEditArgs& a, int b, int nK, int nNew) {
    const int cap = a.cap;
    for (int t = threadIdx.x; t < nNew; t += blockDim.x) {
        const int i = nK + t;
        const double* pr = a.prior + ((long long)b * a.ns + t) * kMapPrior;
        double px = pr[0], py = pr[1], pz = pr[2];
#if defined(__HIP_DEVICE_COMPILE__)
        __asm__ volatile("" : "+v"(px), "+v"(py), "+v"(pz));
#endif
        a.p0[((long long)b * 3 + 0) * cap + i] = px;
        a.p0[((long long)b * 3 + 1) * cap + i] = py;
        a.p0[((long long)b * 3 + 2) * cap + i] = pz;
        a.Q[((long long)b * 5 + 0) * cap + i] = 1.0;
        a.Q[((long long)b * 5 + 1) * cap + i] = 0.0;
        a.Q[((long long)b * 5 + 2) * cap + i] = 0.0;
        a.Q[((long long)b * 5 + 3) * cap + i] = 0.0;
        a.Q[((long long)b * 5 + 4) * cap + i] = 1.0;
        double cst[15];
        int bad = 0;
        landmarkConstants(mk3(px, py, pz), cst, &bad);
        for (int c = 0; c < 15; ++c) a.lmc[((long long)b * 15 + c) * cap + i] = cst[c];
        if (bad && a.errflag) atomicOr(a.errflag, 16);
    }
}

// grid = (ceil(nv / 256), rows, B) over the output of the largest filter (any `rows` >= 1: a workgroup strides over the rows, four in
// flight), block = 256.  Every output entry is written once; the kept part is read once, through the map.
template <typename T>
__global__ __launch_bounds__(256) void k_mapedit_move(MapEditArgs a) {
    const int b = blockIdx.z, tid = threadIdx.x, cap = a.cap;
    const int nK = a.cnt[4 * b], nNew = a.cnt[4 * b + 1], nOld = a.cnt[4 * b + 2];
    const int nvK = kLm0 + 3 * nK, nvn = kLm0 + 3 * (nK + nNew);
    const int* mp = a.map + (long long)b * cap;
    const double* prior = a.prior + (long long)b * a.ns * kMapPrior;
    const T* src = static_cast<const T*>(a.Sin) + (long long)b * a.sigmaStride;
    T* dst = static_cast<T*>(a.Sout) + (long long)b * a.sigmaStride;
    const int ld = a.ld, G = gridDim.y;
    const int Cc = blockIdx.x * 256 + tid;
    if (Cc < nvn) {
        // (the column's source once per thread; the rows' sources are uniform in the workgroup)
        const int Cs = (Cc < kLm0) ? Cc : (Cc < nvK ? kLm0 + 3 * mp[(Cc - kLm0) / 3] + (Cc - kLm0) % 3 : -1);
        // (four rows per trip: their loads are in flight together -- a load behind a store waits for it)
        for (int R0 = blockIdx.y; R0 < nvn; R0 += 4 * G) {
            T v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int R = min(R0 + u * G, nvn - 1);
                if (R < nvK && Cs >= 0) {
                    const int Rs = (R < kLm0) ? R : kLm0 + 3 * mp[(R - kLm0) / 3] + (R - kLm0) % 3;
                    v[u] = src[(long long)Rs * ld + Cs];
                } else {
                    v[u] = mapeditNewEntry<T>(prior, nvK, R, Cc);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (R0 + u * G < nvn) dst[(long long)(R0 + u * G) * ld + Cc] = v[u];
        }
    }
    // ---- per-landmark arrays, one workgroup per filter: compaction through the scratch copy (k_compact's way), then the new landmarks
    if (blockIdx.x != 0 || blockIdx.y != 0) return;
    if (nK == nOld && nNew == 0) return;  // (nothing of this filter changes but the buffer its Sigma lives in)
    if (nK != nOld) {
        for (int i = tid; i < nK; i += blockDim.x) {
            const int o = mp[i];
            double v[kLmRec];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = a.p0[((long long)b * 3 + c) * cap + o];
#pragma unroll
            for (int c = 0; c < 5; ++c) v[3 + c] = a.Q[((long long)b * 5 + c) * cap + o];
#pragma unroll
            for (int c = 0; c < 15; ++c) v[8 + c] = a.lmc[((long long)b * 15 + c) * cap + o];
#pragma unroll
            for (int c = 0; c < kLmRec; ++c) a.scratch[((long long)b * kLmRec + c) * cap + i] = v[c];
        }
        __threadfence_block();
        __syncthreads();  // (every old record has been read: from here on they may be overwritten, by the kept ones and by the new ones)
        for (int i = tid; i < nK; i += blockDim.x) {
            double v[kLmRec];
#pragma unroll
            for (int c = 0; c < kLmRec; ++c) v[c] = a.scratch[((long long)b * kLmRec + c) * cap + i];
#pragma unroll
            for (int c = 0; c < 3; ++c) a.p0[((long long)b * 3 + c) * cap + i] = v[c];
#pragma unroll
            for (int c = 0; c < 5; ++c) a.Q[((long long)b * 5 + c) * cap + i] = v[3 + c];
#pragma unroll
            for (int c = 0; c < 15; ++c) a.lmc[((long long)b * 15 + c) * cap + i] = v[8 + c];
        }
    }
    mapeditWriteNew(a, b, nK, nNew);
    if (tid == 0) a.g[b].N = nK + nNew;
}

// Nobody loses a landmark: filter b = blockIdx.y grows in place by its nNew landmarks (k_append's way: the new rows over all columns, the
// new columns over the old rows, nothing else of Sigma is touched).  grid = (G, B), block = 256; workgroup 0 of a filter writes the landmarks.
template <typename T>
__global__ __launch_bounds__(256) void k_mapedit_append(MapEditArgs a) {
    const int b = blockIdx.y;
    const int nK = a.cnt[4 * b], nNew = a.cnt[4 * b + 1];
    if (nNew == 0) return;
    const int nvK = kLm0 + 3 * nK, nvn = kLm0 + 3 * (nK + nNew), dn = nvn - nvK;
    const double* prior = a.prior + (long long)b * a.ns * kMapPrior;
    T* Sb = static_cast<T*>(a.Sout) + (long long)b * a.sigmaStride;
    const long long nRows = (long long)dn * nvn, total = nRows + (long long)nvK * dn;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        int R, Cc;
        if (e < nRows) {
            R = nvK + (int)(e / nvn);
            Cc = (int)(e % nvn);
        } else {
            const long long f = e - nRows;
            R = (int)(f / dn);
            Cc = nvK + (int)(f % dn);
        }
        Sb[(long long)R * a.ld + Cc] = mapeditNewEntry<T>(prior, nvK, R, Cc);
    }
    if (blockIdx.x != 0) return;
    mapeditWriteNew(a, b, nK, nNew);
    if (threadIdx.x == 0) a.g[b].N = nK + nNew;
}

}  // namespace eqf
