#pragma once
// The covariance downdate Sigma+ = Sigma - Y^T Y (VIOFilter.cpp:297; downdateTile, eqf_update.hpp) of the single-GPU / batched handles on
// the INTEGER matrix pipe -- opt-in, eqf_set_option(f, "downdate_slices", S), S = 5 | 6 | 7; off (fp64) by default.
//
// The same construction as the partitioned filter's eqf_tile_downdate_i8 (eqf_tile.hpp): every column of Y is scaled by a power of two and cut
// into S signed 7-bit slices (|q| <= 64), the slice pairs (ta, tb) with ta + tb < S are multiplied on v_mfma_i32_32x32x32_i8 with EXACT int32
// accumulation (mp * S * 64^2 < 2^31: the host checks it against the handle's capacity) and the S accumulators of an element (one per ta + tb)
// are recombined in fp64.  Lost are the rounding of every entry to the slices (at most 2^-7S of its column's power of two per entry) and the
// dropped slice pairs ta + tb >= S (up to (S - 1) 2^-7S per product term): the rigorous bound and a bit-exact numpy model of these kernels
// are in tests/i8_emulator.py.  Entries are scaled by ldexp(x, -e) each, not times 2^-e (which overflows below 2^-1024).  Six slices keep Sigma within 1e-4 of the fp64 downdate on the bench streams; FIVE do NOT
// (1.4e-4 .. 9e-4 on the partitioned filter) and are accepted for measurement only; seven reach ~1e-8.
//
// Two launches, batched over the filters of a handle (each filter its own nv = kLm0 + 3 N rows / columns of Sigma and mp rows of Y, the rows
// and columns downdateTile reads; column 11 of Y holds z and counts as zero):
//   k_i8dd_split<S>  one workgroup per (32-column tile, filter), two passes over the tile's mp rows: the columns' largest |entry| (-> the
//                    power-of-two exponent), then the slices in the MFMA fragment order of k_i8_split (block ((ct * nKc + kc) * S + t), 1 KB,
//                    lane l: column ct * 32 + (l & 31), rows kc * 32 + 16 (l >> 5) .. + 16).  Exponent word per column: 0 = all zero
//                    (contributes nothing), 1 = holds a NaN / Inf, else frexp's exponent + 2048.  Non-finite entries are NOT sanitised: a
//                    column that holds one makes its row and column of Sigma+ NaN, the pattern the fp64 downdate leaves (x NaN = NaN, also
//                    against the zeros of other columns).  withFinish: one more workgroup per filter runs the innovation lift / group
//                    update (updateFinishBody), as k_downdate's last workgroup does for the per-column launch shapes.
//   k_i8dd_syrk<S>   the upper triangle of 64 x 64 tiles per filter, 4 waves each owning one 32 x 32 MFMA tile with S int32 accumulators;
//                    the fragments come straight from global memory into registers (1 KB per wave and slice, coalesced), one chunk of 32
//                    rows ahead.  Sout = Sin - 2^(e_i + e_j) sum_d acc_d 2^-(12 + 7 d), out of place (the ping-pong of downdateTile); the
//                    element below the diagonal is written from the SAME value as the one above (through LDS, rows as rows): Sigma+ is
//                    exactly symmetric.  A filter with !updateOk || N == 0 copies Sin to Sout.  Tile order: with a batch that is a
//                    multiple of 8 the workgroups of filter b run on XCD b mod 8 and, within an XCD, filter by filter (the rule of
//                    k_chol_resident's downdate tiles, eqf_resident.hpp: filter index fastest streamed every filter's Y from the memory
//                    side again for every tile).
namespace eqf {

typedef int i8ddv4 __attribute__((ext_vector_type(4)));
typedef int i8ddv16 __attribute__((ext_vector_type(16)));
constexpr int kI8ddBits = 7;
constexpr int kI8ddNonFinite = 1;  // exponent word of a column holding a NaN / Inf

struct I8DdArgs {
    const double* Y;          // [B] row-major, ldY, strideY doubles between filters
    int ldY;
    long long strideY;
    const double* Sin;        // [B] nv x nv of ld, sigmaStride doubles between filters
    double* Sout;
    int ld;
    long long sigmaStride;
    const Glob* g;            // filter handles: nv, mp from g[b].N (mp = roundUp(2 N, pad)), copy when !updateOk || N == 0
    const int* dims;          // g == nullptr (eqf_tile_syrk_i8): [B][2] = {nv, mp}, mp == 0 copies
    int pad;
    int skipCol;              // a column of Y that is not part of it (11: z), -1 none
    signed char* ws;          // slices, wsStride bytes per filter
    long long wsStride;
    int* expo;                // exponent words, expoStride per filter
    int expoStride;
    int B, nt;                // filters, 64-wide tiles per edge of the largest filter
};

EQF_DI void i8ddDims(const I8DdArgs& a, int b, int* nv, int* mp) {
    if (a.g) {
        const Glob& g = a.g[b];
        *nv = kLm0 + 3 * g.N;
        *mp = (g.updateOk && g.N != 0) ? roundUp(sDim(g.N), a.pad) : 0;
    } else {
        *nv = a.dims[2 * b];
        *mp = a.dims[2 * b + 1];
    }
}

template <int S>
__global__ __launch_bounds__(256) void k_i8dd_split(I8DdArgs a, UpdArgs u, int withFinish) {
    const int b = blockIdx.y, ct = blockIdx.x;
    if (withFinish && ct == (int)gridDim.x - 1) {
        updateFinishBody(u, b, u.red + (long long)b * 256);
        return;
    }
    int nv, mp;
    i8ddDims(a, b, &nv, &mp);
    if (mp == 0 || ct * 32 >= nv) return;
    const double* Y = a.Y + (long long)b * a.strideY;
    const int tid = threadIdx.x;
    // ---- pass 1: per column the largest |entry| and whether it holds a non-finite one
    {
        const int c = ct * 32 + (tid & 31);
        const bool live = c < nv && c != a.skipCol;
        double mx = 0.0;
        int bad = 0;
        if (live)
            for (int k = tid >> 5; k < mp; k += 8) {
                const double x = Y[(long long)k * a.ldY + c];
                if (!isfinite(x)) bad = 1;
                mx = fmax(mx, fabs(x));
            }
        __shared__ double sMx[8][32];
        __shared__ int sBad[8][32];
        sMx[tid >> 5][tid & 31] = mx;
        sBad[tid >> 5][tid & 31] = bad;
        __syncthreads();
        if (tid < 32) {
#pragma unroll
            for (int r = 1; r < 8; ++r) {
                mx = fmax(mx, sMx[r][tid]);
                bad |= sBad[r][tid];
            }
            int e = 0;
            if (bad) e = kI8ddNonFinite;
            else if (mx > 0.0) {
                frexp(mx, &e);  // mx = f 2^e, f in [0.5, 1): |x| 2^-e < 1
                e += 2048;
            }
            a.expo[(long long)b * a.expoStride + c] = e;
        }
        __syncthreads();
    }
    // ---- pass 2: the slices (as k_i8_split)
    const int nKc = mp / 32, l = tid & 63;
    const int c = ct * 32 + (l & 31);
    const int es = a.expo[(long long)b * a.expoStride + c];  // (written by this workgroup: the barrier above orders it)
    const bool live = c < nv && c != a.skipCol && es > kI8ddNonFinite;
    const int e = live ? es - 2048 : 0;
    int4* out = reinterpret_cast<int4*>(a.ws + (long long)b * a.wsStride);
    for (int kc = tid >> 6; kc < nKc; kc += 4) {
        const int k0 = kc * 32 + (l >> 5) * 16;
        signed char q[S][16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            // |r| < 1, correctly rounded (exact unless it underflows); per entry, not times 2^-e: that factor overflows when e < -1023
            double r = live ? ldexp(Y[(long long)(k0 + j) * a.ldY + c], -e) : 0.0;
            double w = 64.0, wi = 0.015625;                                    // 2^6, then 2^13, 2^20, ...
#pragma unroll
            for (int t = 0; t < S; ++t) {
                const double qq = rint(r * w);  // |qq| <= 64
                q[t][j] = (signed char)(int)qq;
                r = fma(-qq, wi, r);  // exact (wi = 1 / w, a power of two)
                w *= 128.0;
                wi *= 0.0078125;
            }
        }
#pragma unroll
        for (int t = 0; t < S; ++t) {
            int4 v;
            v.x = (unsigned char)q[t][0] | ((unsigned char)q[t][1] << 8) | ((unsigned char)q[t][2] << 16) | ((unsigned)(unsigned char)q[t][3] << 24);
            v.y = (unsigned char)q[t][4] | ((unsigned char)q[t][5] << 8) | ((unsigned char)q[t][6] << 16) | ((unsigned)(unsigned char)q[t][7] << 24);
            v.z = (unsigned char)q[t][8] | ((unsigned char)q[t][9] << 8) | ((unsigned char)q[t][10] << 16) | ((unsigned)(unsigned char)q[t][11] << 24);
            v.w = (unsigned char)q[t][12] | ((unsigned char)q[t][13] << 8) | ((unsigned char)q[t][14] << 16) | ((unsigned)(unsigned char)q[t][15] << 24);
            out[(((long long)ct * nKc + kc) * S + t) * 64 + l] = v;
        }
    }
}

constexpr int kI8ddPitch = 65;
constexpr int kI8ddLdsBytes = 64 * kI8ddPitch * 8;

template <int S>
__global__ __launch_bounds__(256) void k_i8dd_syrk(I8DdArgs a) {
    const int nTiles = a.nt * (a.nt + 1) / 2;
    const int w = blockIdx.x;
    int b, tile;
    if ((a.B & 7) == 0) {  // workgroup w runs on XCD w mod 8: there, filter by filter
        const int seq = w >> 3;
        b = (w & 7) + 8 * (seq / nTiles);
        tile = seq % nTiles;
    } else {
        b = w / nTiles;
        tile = w % nTiles;
    }
    int ti = 0, rem = tile;
    while (rem >= a.nt - ti) {
        rem -= a.nt - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int I0 = ti * 64, J0 = tj * 64;
    int nv, mp;
    i8ddDims(a, b, &nv, &mp);
    if (J0 >= nv) return;  // (I0 <= J0)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const double* Sin = a.Sin + (long long)b * a.sigmaStride;
    double* Sout = a.Sout + (long long)b * a.sigmaStride;
    if (mp == 0) {
        for (int e = tid; e < 64 * 64; e += 256) {
            const int R = I0 + (e >> 6), Cc = J0 + (e & 63);
            if (R < nv && Cc < nv) {
                Sout[(long long)R * a.ld + Cc] = Sin[(long long)R * a.ld + Cc];
                if (ti != tj) Sout[(long long)Cc * a.ld + R] = Sin[(long long)Cc * a.ld + R];
            }
        }
        return;
    }
    const int nKc = mp / 32, nCt = (nv + 31) / 32;
    const int ctA = 2 * ti + wr, ctB = 2 * tj + wc;
    i8ddv16 acc[S];
#pragma unroll
    for (int d = 0; d < S; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[d][r] = 0;
    if (ctA < nCt && ctB < nCt) {  // (wave-uniform: a 32-column tile past nv has no slices)
        const int4* ws = reinterpret_cast<const int4*>(a.ws + (long long)b * a.wsStride);
        const int4* gA = ws + (long long)ctA * nKc * S * 64 + lane;
        const int4* gB = ws + (long long)ctB * nKc * S * 64 + lane;
        int4 na[S], nb[S];
#pragma unroll
        for (int t = 0; t < S; ++t) {
            na[t] = gA[t * 64];
            nb[t] = gB[t * 64];
        }
        for (int kc = 0; kc < nKc; ++kc) {
            i8ddv4 fa[S], fb[S];
#pragma unroll
            for (int t = 0; t < S; ++t) {
                fa[t] = i8ddv4{na[t].x, na[t].y, na[t].z, na[t].w};
                fb[t] = i8ddv4{nb[t].x, nb[t].y, nb[t].z, nb[t].w};
            }
            if (kc + 1 < nKc) {
#pragma unroll
                for (int t = 0; t < S; ++t) {
                    na[t] = gA[((long long)(kc + 1) * S + t) * 64];
                    nb[t] = gB[((long long)(kc + 1) * S + t) * 64];
                }
            }
#pragma unroll
            for (int ta = 0; ta < S; ++ta)
#pragma unroll
                for (int tb = 0; tb + ta < S; ++tb) acc[ta + tb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[ta], fb[tb], acc[ta + tb], 0, 0, 0);
        }
    }
    // ---- epilogue: the fp64 downdate term of every element into LDS, then Sout row by row (upper part), then the mirror from the same values
    extern __shared__ __attribute__((aligned(16))) unsigned char sBufI8dd[];
    double (*sD)[kI8ddPitch] = reinterpret_cast<double (*)[kI8ddPitch]>(sBufI8dd);
    const int* ex = a.expo + (long long)b * a.expoStride;
    const int jl = 32 * wc + (lane & 31), j = J0 + jl;
    const int ej = j < nv ? ex[j] : 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int il = 32 * wr + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), i = I0 + il;
        const int ei = i < nv ? ex[i] : 0;
        double dv = 0.0;
        if (ei == kI8ddNonFinite || ej == kI8ddNonFinite) {
            dv = __builtin_nan("");
        } else if (ei != 0 && ej != 0) {  // (a column that is all zero contributes nothing)
            double v = 0.0;
#pragma unroll
            for (int d = S - 1; d >= 0; --d) v += ldexp((double)acc[d][r], -(12 + kI8ddBits * d));  // smallest terms first
            dv = ldexp(v, ei - 2048 + ej - 2048);
        }
        sD[il][jl] = dv;
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
        const int r = e >> 6, cc = e & 63, R = I0 + r, Cc = J0 + cc;
        if (R < nv && Cc < nv && R <= Cc) {
            const double v = Sin[(long long)R * a.ld + Cc] - sD[r][cc];
            Sout[(long long)R * a.ld + Cc] = v;
            sD[r][cc] = v;
        }
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
        const int r = e >> 6, cc = e & 63, R = J0 + r, Cc = I0 + cc;  // row in the J range, column in the I range
        if (R < nv && Cc < nv && R > Cc) Sout[(long long)R * a.ld + Cc] = sD[cc][r];
    }
}

// Workspace of the slices per filter (capacity nvCap x mpCap), in bytes; exponent words per filter
inline long long i8ddSliceBytes(int nvCap, int mpCap, int S) { return (long long)((nvCap + 31) / 32) * (mpCap / 32) * S * 1024; }
inline int i8ddExpoWords(int nvCap) { return (nvCap + 31) / 32 * 32; }
// int32 accumulation stays exact: an accumulator sums at most S slice products of |q| <= 64 per row
inline bool i8ddExact(int mpCap, int S) { return (long long)mpCap * S * 64 * 64 < (1LL << 31); }

template <int S>
void launchI8Dd(const I8DdArgs& a, const UpdArgs* u, int nCt, hipStream_t st) {
    UpdArgs uu{};
    if (u) uu = *u;
    hipLaunchKernelGGL((k_i8dd_split<S>), dim3(nCt + (u ? 1 : 0), a.B), dim3(256), 0, st, a, uu, u ? 1 : 0);
    hipLaunchKernelGGL((k_i8dd_syrk<S>), dim3(a.nt * (a.nt + 1) / 2 * a.B), dim3(256), kI8ddLdsBytes, st, a);
}
// u != nullptr: the innovation lift rides along in the split launch (the per-column launch shapes; k_chol_resident ran it in its roles)
inline void launchI8DdS(int S, const I8DdArgs& a, const UpdArgs* u, int nCt, hipStream_t st) {
    if (S == 5) launchI8Dd<5>(a, u, nCt, st);
    else if (S == 6) launchI8Dd<6>(a, u, nCt, st);
    else launchI8Dd<7>(a, u, nCt, st);
}

}  // namespace eqf
