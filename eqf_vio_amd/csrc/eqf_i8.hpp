#pragma once
// The int8-slice products: C -= A^T B on the INTEGER matrix pipe, opt-in with 5, 6 or 7 slices (off -- fp64 -- by default).  Two users:
// the partitioned filter's downdate and trailing products (eqf_tile_downdate_i8 / eqf_tile_gemm_tn_i8, eqf_tiled.hip; eqf_tf_set_option
// "downdate_slices" / "chain_slices") and the single-GPU / batched handles' downdate Sigma - Y^T Y (eqf_set_option "downdate_slices",
// eqf_tile_syrk_i8, eqf_capi.hip).  Both run the same construction:
//   1. per column an exponent word (i8ExpoWord): 0 = all zero (contributes nothing), kI8NonFinite = holds a NaN / Inf (its row / column of
//      the result is NaN, as fp64 gives: x NaN and Inf x 0 are NaN -- non-finite entries are never sanitised), else e + kI8Bias for
//      frexp's exponent e of the largest |entry|;
//   2. every entry scaled by ldexp(x, -e) (|r| < 1, correctly rounded; a factor 2^-e would overflow below 2^-1024) and cut into S signed
//      7-bit slices q_t = rint(r 2^(6 + 7 t)), |q_t| <= 64, r -= q_t 2^-(6 + 7 t) exactly (i8SliceEntry, i8StoreLane), stored in MFMA FRAGMENT order:
//      for a 32-column tile ct, a 32-row chunk kc and slice t one 1 KB block (i8Frag) whose lane l holds column ct * 32 + (l & 31), rows
//      kc * 32 + 16 (l >> 5) .. + 16 -- the operand layout of v_mfma_i32_32x32x32_i8;
//   3. the S (S + 1) / 2 slice pairs (ta, tb) with ta + tb < S multiplied on v_mfma_i32_32x32x32_i8 into S int32 accumulators, one per
//      ta + tb (i8Mfma).  EXACT while rows * S * 64^2 < 2^31 (i8Exact): the tile entry points refuse k > 70 000, the handles a capacity above
//      ~37 000;
//   4. recombined in fp64 (i8Term): ldexp(sum_d acc_d 2^-(12 + 7 d), e_i + e_j), the smallest terms first.
// Error: the rounding of every entry to its slices (at most 2^-7S of its column's 2^e) and the dropped pairs ta + tb >= S (up to
// (S - 1) 2^-7S per product term), so |error_ij| <= about k 2^(e_i + e_j) (S + 1) 2^-7S.  tests/i8_emulator.py derives the rigorous bound and
// models every kernel here operation for operation; tests/test_gpu_i8_exact.py holds the kernels to it bit for bit.  Random data stay well
// inside the bound; inputs whose digits all share a sign come close (an older "k ca cb 2^-(5 + 7 (S - 1))" bound is exceeded by 1.5x there).
// Accuracy in the filters (bench streams: scripts/slice_precision_study*.py, profiles/r06_slice_precision_study*.txt,
// profiles/r06_i8_downdate_error.txt): the truncation alone would allow S = 5, but the dropped pairs add up coherently over Y's correlated
// columns.  Downdate, Sigma against the fp64 path: S = 5: 1.4e-4 .. 9e-4 (misses 1e-4: for measurement only), S = 6: 2e-6 .. 6e-5, S = 7:
// 1e-8 .. 8e-8.  The factorisations' trailing products forgive more (subtracted from S and Sigma_e, averaged by K over 2 N rows): S = 5
// keeps Sigma to 1e-8 and the pose to 3e-9.
//
// The partitioned filter (one operand pair per call; the host cuts A once when it is a column range of B):
//   k_i8_zero, k_i8_colexp  the exponent words: zeroed, then an atomicMax over row slabs of 512 (kI8NonFinite wins it)
//   k_i8_split<S>           the slices, a wave per 32-row chunk of a 32-column tile; rows past k and columns past m are zero
//   k_i8_gemm<S>            512 threads = 8 waves as 4 x 2, workgroup tile 128 (rows of C) x 64, a wave owns ONE 32 x 32 MFMA tile (two waves
//                           per SIMD); a chunk's 6 S fragment blocks go global -> LDS directly (global_load_lds_dwordx4: the global layout IS
//                           the LDS image), three LDS buffers (chunk kc + 2 in flight while kc is multiplied), one raw s_barrier per chunk
//                           behind a counted vmcnt.  mk.rb > 0: the first maskCols columns of C are masked as in k_tile_gemm_tn (tiles
//                           entirely below the block diagonal are skipped); columns from maskCols on (right-hand sides) are always formed.
//                           C[i][j] += alpha * term.
//   Measured (scripts/micro/i8_split_gemm.hip, profiles/r06_i8_split_gemm_v2.txt): S = 5: 84 - 108 fp64-equivalent TFLOP/s at the downdate's
//   shapes (1.3 - 1.6 POPS of int8) against 51 - 57 for k_tile_gemm_tn in the same run.
// The handles (batched over the filters of a handle, each its own nv = kLm0 + 3 N rows / columns of Sigma and mp rows of Y, the rows and
// columns downdateTile reads; column 11 of Y holds z and counts as zero):
//   k_i8dd_split<S>  one workgroup per (32-column tile, filter), two passes over the tile's mp rows: the exponent words, then the slices.
//                    withFinish: one more workgroup per filter runs the innovation lift / group update (updateFinishBody), as k_downdate's
//                    last workgroup does for the per-column launch shapes.
//   k_i8dd_syrk<S>   the upper triangle of 64 x 64 tiles per filter, 4 waves each owning one 32 x 32 MFMA tile; the fragments come straight
//                    from global memory into registers (1 KB per wave and slice, coalesced), one chunk of 32 rows ahead.  Sout = Sin - term,
//                    out of place (the ping-pong of downdateTile); the element below the diagonal is written from the SAME value as the one
//                    above (through LDS, rows as rows): Sigma+ is exactly symmetric.  A filter with !updateOk || N == 0 copies Sin to Sout.
//                    Tile order: with a batch that is a multiple of 8 the workgroups of filter b run on XCD b mod 8 and, within an XCD,
//                    filter by filter (the rule of k_chol_resident's downdate tiles, eqf_resident.hpp: filter index fastest streamed every
//                    filter's Y from the memory side again for every tile).
// The two split kernels and the two product kernels differ for measured speed reasons (DESIGN.md sections 2 and 4.5).
#include <type_traits>
#include "eqf_update.hpp"

namespace eqf {

typedef int i8v4 __attribute__((ext_vector_type(4)));
typedef int i8v16 __attribute__((ext_vector_type(16)));
constexpr int kI8Bits = 7;          // bits per slice
constexpr int kI8Bias = 2048;       // exponent word = frexp's exponent + kI8Bias (<= 3072)
constexpr int kI8NonFinite = 4096;  // exponent word of a column holding a NaN / Inf: above every biased exponent, so it wins k_i8_colexp's atomicMax

// int32 accumulation stays exact: an accumulator sums at most S slice products of |q| <= 64 per row
constexpr bool i8Exact(long long rows, int S) { return rows * S * 64 * 64 < (1LL << 31); }
constexpr int kI8MaxK = 70000;  // the tile entry points' k limit
static_assert(i8Exact(kI8MaxK, 7), "k_i8_gemm's int32 accumulators must stay exact up to kI8MaxK rows");
// bytes of the slices of an operand of `rows` x `cols` (1 KB per 32-column tile, 32-row chunk and slice)
inline long long i8SliceBytes(int rows, int cols, int S) { return (long long)((cols + 31) / 32) * ((rows + 31) / 32) * S * 1024; }
// f(std::integral_constant<int, S>{}) for S = slices (5, 6 or 7: the callers have checked)
template <typename F>
auto i8WithSlices(int slices, F&& f) {
    if (slices == 5) return f(std::integral_constant<int, 5>{});
    if (slices == 6) return f(std::integral_constant<int, 6>{});
    return f(std::integral_constant<int, 7>{});
}

EQF_DI int i8ExpoWord(double mx, bool nonFinite) {
    if (nonFinite) return kI8NonFinite;
    if (!(mx > 0.0)) return 0;
    int e = 0;
    frexp(mx, &e);  // mx = f 2^e, f in [0.5, 1): |x| 2^-e < 1
    return e + kI8Bias;
}
EQF_DI bool i8Live(int word) { return word > 0 && word != kI8NonFinite; }  // (a flagged column is cut as zeros: the epilogue writes NaN for it)
// int4 index of `lane` in fragment block (ct, kc, t) of a slice buffer with nKc chunks
EQF_DI long long i8Frag(int ct, int nKc, int kc, int S, int t, int lane) { return (((long long)ct * nKc + kc) * S + t) * 64 + lane; }

// entry j of a lane's 16 rows, scaled (|r| < 1), cut into its S slices q[t][j]
template <int S>
__device__ __forceinline__ void i8SliceEntry(double r, signed char (&q)[S][16], int j) {
    double w = 64.0, wi = 0.015625;  // 2^6, then 2^13, 2^20, ...
#pragma unroll
    for (int t = 0; t < S; ++t) {
        const double qq = rint(r * w);  // |qq| <= 64
        q[t][j] = (signed char)(int)qq;
        r = fma(-qq, wi, r);  // exact (wi = 1 / w, a power of two)
        w *= 128.0;
        wi *= 0.0078125;
    }
}
// the lane's slices in fragment order: slice t to out[t * 64], byte j = row j
template <int S>
__device__ __forceinline__ void i8StoreLane(const signed char (&q)[S][16], int4* out) {
#pragma unroll
    for (int t = 0; t < S; ++t) {
        int4 v;
        v.x = (unsigned char)q[t][0] | ((unsigned char)q[t][1] << 8) | ((unsigned char)q[t][2] << 16) | ((unsigned)(unsigned char)q[t][3] << 24);
        v.y = (unsigned char)q[t][4] | ((unsigned char)q[t][5] << 8) | ((unsigned char)q[t][6] << 16) | ((unsigned)(unsigned char)q[t][7] << 24);
        v.z = (unsigned char)q[t][8] | ((unsigned char)q[t][9] << 8) | ((unsigned char)q[t][10] << 16) | ((unsigned)(unsigned char)q[t][11] << 24);
        v.w = (unsigned char)q[t][12] | ((unsigned char)q[t][13] << 8) | ((unsigned char)q[t][14] << 16) | ((unsigned)(unsigned char)q[t][15] << 24);
        out[t * 64] = v;
    }
}

template <int S>
__device__ __forceinline__ void i8Clear(i8v16 (&acc)[S]) {
#pragma unroll
    for (int d = 0; d < S; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[d][r] = 0;
}
// the slice pairs ta + tb < S of one 32-row chunk
template <int S>
__device__ __forceinline__ void i8Mfma(i8v16 (&acc)[S], const i8v4 (&a)[S], const i8v4 (&b)[S]) {
#pragma unroll
    for (int ta = 0; ta < S; ++ta)
#pragma unroll
        for (int tb = 0; tb + ta < S; ++tb) acc[ta + tb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ta], b[tb], acc[ta + tb], 0, 0, 0);
}
// the term of element (i, j) from entry r of its accumulators, exponent words wi / wj: false = nothing (a column is all zero)
template <int S>
__device__ __forceinline__ bool i8Term(const i8v16 (&acc)[S], int r, int wi, int wj, double* term) {
    if (wi == kI8NonFinite || wj == kI8NonFinite) {
        *term = __builtin_nan("");  // (as fp64: x NaN / Inf poisons the element)
    } else if (wi != 0 && wj != 0) {
        double v = 0.0;
#pragma unroll
        for (int d = S - 1; d >= 0; --d) v += ldexp((double)acc[d][r], -(12 + kI8Bits * d));  // smallest terms first
        *term = ldexp(v, wi - kI8Bias + wj - kI8Bias);
    } else {
        return false;
    }
    return true;
}

// ---- the partitioned filter's kernels (inline: this header is read by two translation units)
__global__ __launch_bounds__(256) inline void k_i8_colexp(const double* X, int K, int M, int ld, int* expo) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), kq = threadIdx.x >> 6;
    const int k0 = blockIdx.y * 512, k1 = min(k0 + 512, K);
    double mx = 0.0;
    if (c < M)
        for (int k = k0 + kq; k < k1; k += 4) {
            const double x = X[(long long)k * ld + c];
            mx = fmax(mx, isfinite(x) ? fabs(x) : INFINITY);  // (fmax drops a NaN: a non-finite entry counts as +Inf)
        }
    __shared__ double sm[4][64];
    sm[kq][threadIdx.x & 63] = mx;
    __syncthreads();
    if (kq == 0 && c < M) {
        mx = fmax(fmax(sm[0][threadIdx.x], sm[1][threadIdx.x]), fmax(sm[2][threadIdx.x], sm[3][threadIdx.x]));
        const int w = i8ExpoWord(mx, mx == INFINITY);
        if (w != 0) atomicMax(expo + c, w);
    }
}

__global__ __launch_bounds__(256) inline void k_i8_zero(int* p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

template <int S>
__global__ __launch_bounds__(256) void k_i8_split(const double* X, int K, int M, int ld, const int* expo, signed char* out, int nKc) {
    const int ct = blockIdx.x, kc = blockIdx.y * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (kc >= nKc) return;
    const int c = ct * 32 + (l & 31), k0 = kc * 32 + (l >> 5) * 16;
    const int es = c < M ? expo[c] : 0;
    const bool live = c < M && i8Live(es);
    const int e = live ? es - kI8Bias : 0;
    signed char q[S][16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = k0 + j;
        // |r| < 1, correctly rounded (exact unless it underflows); per entry, not times 2^-e: that factor overflows when e < -1023
        i8SliceEntry<S>((live && k < K) ? ldexp(X[(long long)k * ld + c], -e) : 0.0, q, j);
    }
    i8StoreLane<S>(q, reinterpret_cast<int4*>(out) + i8Frag(ct, nKc, kc, S, 0, l));
}

typedef const void __attribute__((address_space(1)))* i8gptr_t;
typedef void __attribute__((address_space(3)))* i8lptr_t;
template <int S>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_i8_gemm(const signed char* As, const signed char* Bs,
    const int* eA, const int* eB, double* C, int M, int N, int ldc, int nKc, double alpha, GemmMask mk, int maskCols) {
    constexpr int kFrag = 6 * S, kPerWave = (kFrag + 7) / 8, kSlots = kPerWave * 8;  // (every wave issues the same number of copies: one vmcnt)
    __shared__ int4 sm[3][kSlots * 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const int ctA0 = blockIdx.y * 4, ctB0 = blockIdx.x * 2;
    if (mk.rb > 0 && ctB0 * 32 + 63 < maskCols) {  // (uniform) a tile inside the masked columns, entirely below the block diagonal: nobody reads it
        const int Ilo = (mk.rblk0 + (ctA0 * 32) / mk.rb) * mk.Pr + mk.pr;
        const int Jhi = (mk.cblk0 + (ctB0 * 32 + 63) / mk.cb) * mk.Pc + mk.pc;
        if (Ilo > Jhi) return;
    }
    const int4* gA = reinterpret_cast<const int4*>(As);
    const int4* gB = reinterpret_cast<const int4*>(Bs);
    auto stage = [&](int kc, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kPerWave; ++j) {
            const int slot = wv + 8 * j;
            const int blk = slot < kFrag ? slot : 0;  // (pad slots re-read block 0 into LDS nobody looks at)
            const int4* src;
            if (blk < 4 * S) {
                const int ct = blk / S, t = blk - ct * S;
                src = gA + i8Frag(ctA0 + ct, nKc, kc, S, t, lane);
            } else {
                const int b2 = blk - 4 * S, ct = b2 / S, t = b2 - ct * S;
                src = gB + i8Frag(ctB0 + ct, nKc, kc, S, t, lane);
            }
            __builtin_amdgcn_global_load_lds((i8gptr_t)src, (i8lptr_t)&sm[buf][slot * 64], 16, 0, 0);
        }
    };
    i8v16 acc[S];
    i8Clear<S>(acc);
    stage(0, 0);
    if (nKc > 1) stage(1, 1);
    // chunk 0 complete (the older kPerWave of this wave's copies), then everybody's: the barrier
    if (nKc > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPerWave) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int kc = 0; kc < nKc; ++kc) {
        const int buf = kc % 3;
        if (kc + 2 < nKc) stage(kc + 2, (kc + 2) % 3);  // (that buffer was read in iteration kc - 1: the barrier at its end has been passed)
        i8v4 a[S], b[S];
#pragma unroll
        for (int t = 0; t < S; ++t) {
            const int4 va = sm[buf][(wr * S + t) * 64 + lane];
            const int4 vb = sm[buf][(4 * S + wc * S + t) * 64 + lane];
            a[t] = i8v4{va.x, va.y, va.z, va.w};
            b[t] = i8v4{vb.x, vb.y, vb.z, vb.w};
        }
        i8Mfma<S>(acc, a, b);
        // chunk kc + 1 must be in LDS before anybody reads it: this wave's copies of it are the older ones of what it has in flight; and
        // every read of this chunk has returned before its buffer is restaged two iterations on
        if (kc + 2 < nKc) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPerWave) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    const int j = (ctB0 + wc) * 32 + (lane & 31);
    const int ibase = (ctA0 + wr) * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = ibase + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        double t;
        if (i < M && j < N && i8Term<S>(acc, r, eA[i], eB[j], &t)) C[(long long)i * ldc + j] += alpha * t;
    }
}

// ---- the handles' kernels
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
            a.expo[(long long)b * a.expoStride + c] = i8ExpoWord(mx, bad);
        }
        __syncthreads();
    }
    // ---- pass 2: the slices
    const int nKc = mp / 32, l = tid & 63;
    const int c = ct * 32 + (l & 31);
    const int es = a.expo[(long long)b * a.expoStride + c];  // (written by this workgroup: the barrier above orders it)
    const bool live = c < nv && c != a.skipCol && i8Live(es);
    const int e = live ? es - kI8Bias : 0;
    int4* out = reinterpret_cast<int4*>(a.ws + (long long)b * a.wsStride);
    for (int kc = tid >> 6; kc < nKc; kc += 4) {
        const int k0 = kc * 32 + (l >> 5) * 16;
        signed char q[S][16];
#pragma unroll
        for (int j = 0; j < 16; ++j) i8SliceEntry<S>(live ? ldexp(Y[(long long)(k0 + j) * a.ldY + c], -e) : 0.0, q, j);
        i8StoreLane<S>(q, out + i8Frag(ct, nKc, kc, S, 0, l));
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
    i8v16 acc[S];
    i8Clear<S>(acc);
    if (ctA < nCt && ctB < nCt) {  // (wave-uniform: a 32-column tile past nv has no slices)
        const int4* ws = reinterpret_cast<const int4*>(a.ws + (long long)b * a.wsStride);
        const int4* gA = ws + i8Frag(ctA, nKc, 0, S, 0, lane);
        const int4* gB = ws + i8Frag(ctB, nKc, 0, S, 0, lane);
        int4 na[S], nb[S];
#pragma unroll
        for (int t = 0; t < S; ++t) {
            na[t] = gA[t * 64];
            nb[t] = gB[t * 64];
        }
        for (int kc = 0; kc < nKc; ++kc) {
            i8v4 fa[S], fb[S];
#pragma unroll
            for (int t = 0; t < S; ++t) {
                fa[t] = i8v4{na[t].x, na[t].y, na[t].z, na[t].w};
                fb[t] = i8v4{nb[t].x, nb[t].y, nb[t].z, nb[t].w};
            }
            if (kc + 1 < nKc) {
#pragma unroll
                for (int t = 0; t < S; ++t) {
                    na[t] = gA[((long long)(kc + 1) * S + t) * 64];
                    nb[t] = gB[((long long)(kc + 1) * S + t) * 64];
                }
            }
            i8Mfma<S>(acc, fa, fb);
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
        double dv = 0.0;
        i8Term<S>(acc, r, i < nv ? ex[i] : 0, ej, &dv);
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

// exponent words per filter of capacity nvCap
inline int i8ddExpoWords(int nvCap) { return (nvCap + 31) / 32 * 32; }

}  // namespace eqf
