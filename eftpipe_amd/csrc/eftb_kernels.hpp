// eftb_kernels.hpp -- HIP kernels of the one-loop engine, written for gfx950 (MI355X, CDNA4) only.
//
// Everything is FP64.  The one-loop double sums (P22, C22, C13) are regrouped by anti-diagonals into one k-independent
// pass per cosmology plus a 513-term synthesis per output point; the syntheses, the IR-resummation polynomials and the
// post-AP projection operators run on the FP64 matrix cores (v_mfma_f64_16x16x4_f64).  The remaining stages are small
// streaming kernels (spline sweeps, prefix sums, wave reductions).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace eftb {

constexpr int NS = 80;       // |sbird|                         reference pybird.py:481-482
constexpr int NPOW = 257;    // FFTLog powers (NFFT + 1)         reference pybird.py:919
constexpr int NHALF = 128;
constexpr int NCH = 129;     // independent complex coefficients

constexpr int NROW = 24;     // template rows per multipole: 3 (P11l) + 6 (Pctl) + 12 (Ploopl) + 3 (Pstl)

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

// Flat workgroup id -> (tile, group) such that the `ntile` tiles of one group (the k tiles of one cosmology / of one share of the series) run
// on ONE XCD: consecutive workgroup ids go round the eight XCDs, each with its own L2, so with the plain (tile fastest) order every k tile of
// a cosmology sits on a different XCD and whatever the tiles share (halo windows, per-cosmology tables) is fetched from HBM once per tile.
__device__ __forceinline__ void xcd_decode(int ntile, int& tile, int& group) {
    const int flat = blockIdx.x, ng = gridDim.x / ntile;
    if ((ng & 7) == 0) {
        const int slot = flat >> 3;
        tile = slot % ntile;
        group = (flat & 7) + 8 * (slot / ntile);
    } else {
        tile = flat % ntile;
        group = flat / ntile;
    }
}

// ------------------------------------------------------------------------------------------------
// First stage.  P11 = Sk Pin (cubic spline kin -> k), the 129 independent FFTLog coefficients = G Pin + E tail(slope, amp) and the IR
// filters X, Y = B Pin + T tail'(slope', amp') are fixed real operators on the 200 input samples and on the power-law tails that continue
// them (reference pybird.py:694-695, fftlog.py:84-166, pybird.py:1316-1353).  With the batch as the row dimension they are small GEMMs on
// the matrix cores (gemm_direct_kernel), whose tables are read once per 16 cosmologies instead of once per cosmology.
// prep_rows_kernel writes the operand rows: A1 = Pin (for P11), A2 = [Pin | tail] (coefficients; also transposed, for the
// cosmology-contiguous copy the anti-diagonal pass reads), A3 = [Pin | tail'] (IR filters), zero padded to multiples of the GEMM's K chunk.
// One workgroup per cosmology.  A1 / A3 may be null (only the other part is wanted).  Input guard: include/eftbird.h.
// Input grids that start above the FFTLog's xmin (LO = true): the last ntail_lo / nxtail_lo columns of A2 / A3 continue the function at the low end
// as well, with the slope and amplitude of ITS first two samples (reference fftlog.py:140-145); wq2 then holds 4 weights (last two, first two).
// ------------------------------------------------------------------------------------------------
template <bool LO>
__device__ __forceinline__ void prep_rows_body(int Nkin, int ntail, int nxtail, int KP1, int KP2, int KP3, int Bmax,
                                                        const double* __restrict__ Pin, const double* __restrict__ lnkin,
                                                        const double* __restrict__ lnxtail, const double* __restrict__ lnxxtail,
                                                        const double* __restrict__ wq2, double* __restrict__ A1, double* __restrict__ A2,
                                                        double* __restrict__ A2T, double* __restrict__ A3, int* __restrict__ status,
                                                        int ntail_lo, int nxtail_lo) {
    extern __shared__ double sm[];
    double* pin = sm;
    const int w = blockIdx.x, tid = threadIdx.x;
    bool bad = false;
    for (int j = tid; j < Nkin; j += blockDim.x) {
        const double v = Pin[(size_t)w * Nkin + j];
        pin[j] = v;
        bad = bad || !(fabs(v) <= 1.79769313486231570815e308) || (j >= Nkin - 2 && !(v > 0.0));  // non-finite anywhere, non-positive where the logarithm is taken
        if (LO) bad = bad || (j < 2 && !(v > 0.0));                                                 // (the low tails take it of the first two as well)
    }
    // input guard (reference fftlog.py:146-151 needs the last two samples positive): the flag sits in mapped host memory and is only written in the error case
    if (bad && status) atomicMax(status, w + 1);
    __syncthreads();
    const double dln = lnkin[Nkin - 1] - lnkin[Nkin - 2];
    const double dlo = LO ? lnkin[1] - lnkin[0] : 0.0;
    if (A1) {
        // slope / amplitude from the last two samples (reference fftlog.py:146-151)
        const double slope = (log(pin[Nkin - 1]) - log(pin[Nkin - 2])) / dln;
        const double amp = pin[Nkin - 1] * exp(-slope * lnkin[Nkin - 1]);
        double slo = 0.0, alo = 0.0;
        if (LO && ntail_lo) {  // ... and from the first two (fftlog.py:140-145)
            slo = (log(pin[1]) - log(pin[0])) / dlo;
            alo = pin[0] * exp(-slo * lnkin[0]);
        }
        const int nhi = ntail - (LO ? ntail_lo : 0);
        for (int j = tid; j < KP1; j += blockDim.x) A1[(size_t)w * KP1 + j] = j < Nkin ? pin[j] : 0.0;
        for (int j = tid; j < KP2; j += blockDim.x) {
            double v = j < Nkin ? pin[j] : (j < Nkin + ntail ? amp * exp(slope * lnxtail[j - Nkin]) : 0.0);
            if (LO && j >= Nkin + nhi && j < Nkin + ntail) v = alo * exp(slo * lnxtail[j - Nkin]);
            A2[(size_t)w * KP2 + j] = v;
            A2T[(size_t)j * Bmax + w] = v;
        }
    }
    if (A3) {
        // the IR filters act on q = Pin exp(-k^2 / Lambda^2) / k^2 (the weight is folded into the operator); the tail continues q's last two samples
        const double q1 = pin[Nkin - 1] * wq2[1], q0 = pin[Nkin - 2] * wq2[0];
        const double slope = (log(q1) - log(q0)) / dln;
        const double amp = q1 * exp(-slope * lnkin[Nkin - 1]);
        double slo = 0.0, alo = 0.0;
        if (LO && nxtail_lo) {  // the low tail continues q's first two samples
            const double p0 = pin[0] * wq2[2], p1 = pin[1] * wq2[3];
            slo = (log(p1) - log(p0)) / dlo;
            alo = p0 * exp(-slo * lnkin[0]);
        }
        const int nhi = nxtail - (LO ? nxtail_lo : 0);
        for (int j = tid; j < KP3; j += blockDim.x) {
            double v = j < Nkin ? pin[j] : (j < Nkin + nxtail ? amp * exp(slope * lnxxtail[j - Nkin]) : 0.0);
            if (LO && j >= Nkin + nhi && j < Nkin + nxtail) v = alo * exp(slo * lnxxtail[j - Nkin]);
            A3[(size_t)w * KP3 + j] = v;
        }
    }
}

#define PREP_ROWS_PARAMS int Nkin, int ntail, int nxtail, int KP1, int KP2, int KP3, int Bmax, const double* __restrict__ Pin, \
    const double* __restrict__ lnkin, const double* __restrict__ lnxtail, const double* __restrict__ lnxxtail, const double* __restrict__ wq2, \
    double* __restrict__ A1, double* __restrict__ A2, double* __restrict__ A2T, double* __restrict__ A3, int* __restrict__ status
#define PREP_ROWS_ARGS Nkin, ntail, nxtail, KP1, KP2, KP3, Bmax, Pin, lnkin, lnxtail, lnxxtail, wq2, A1, A2, A2T, A3, status

__global__ __launch_bounds__(256) void prep_rows_kernel(PREP_ROWS_PARAMS) {
    prep_rows_body<false>(PREP_ROWS_ARGS, 0, 0);
}

__global__ __launch_bounds__(256) void prep_rows_lo_kernel(PREP_ROWS_PARAMS, int ntail_lo, int nxtail_lo) {
    prep_rows_body<true>(PREP_ROWS_ARGS, ntail_lo, nxtail_lo);
}

// Q(f) of Resum.makeQ for one cosmology (qf_kernel's body; declared here for the merged front launch below)
__device__ __forceinline__ void qf_body(int w, int nq, const double* __restrict__ fgrow, const double* __restrict__ Qpoly, double* __restrict__ Q) {
    const int tid = threadIdx.x;
    const double f = fgrow[w];
    for (int idx = tid; idx < 2 * nq; idx += blockDim.x) {
        const int a = idx / nq, rest = idx % nq;
        const double* c = Qpoly + ((size_t)(1 - a) * nq + rest) * 15;
        double cv[15];
#pragma unroll
        for (int p = 0; p < 15; ++p) cv[p] = c[p];
        const double f2 = f * f;
        double ev = cv[14], od = cv[13];  // even / odd powers: two chains
#pragma unroll
        for (int p = 12; p >= 0; p -= 2) {
            ev = fma(ev, f2, cv[p]);
            if (p >= 1) od = fma(od, f2, cv[p - 1]);
        }
        Q[(size_t)w * 2 * nq + idx] = fma(od, f, ev);
    }
}

// operand rows and Q(f) in one launch (direct-P_l runs: both are the first kernels of the front on the side stream; a launch costs the host
// 4 us and the step is bounded by the host): workgroups [0, B) = prep_rows, [B, 2 B) = Q(f)
__global__ __launch_bounds__(256) void prep_rows_qf_kernel(int B, PREP_ROWS_PARAMS, int nq, const double* __restrict__ fgrow,
                                                           const double* __restrict__ Qpoly, double* __restrict__ Q) {
    if ((int)blockIdx.x >= B) {
        qf_body(blockIdx.x - B, nq, fgrow, Qpoly, Q);
        return;
    }
    prep_rows_body<false>(PREP_ROWS_ARGS, 0, 0);
}

__global__ __launch_bounds__(256) void prep_rows_qf_lo_kernel(int B, PREP_ROWS_PARAMS, int nq, const double* __restrict__ fgrow,
                                                              const double* __restrict__ Qpoly, double* __restrict__ Q, int ntail_lo, int nxtail_lo) {
    if ((int)blockIdx.x >= B) {
        qf_body(blockIdx.x - B, nq, fgrow, Qpoly, Q);
        return;
    }
    prep_rows_body<true>(PREP_ROWS_ARGS, ntail_lo, nxtail_lo);
}
#undef PREP_ROWS_PARAMS
#undef PREP_ROWS_ARGS

// ------------------------------------------------------------------------------------------------
// One-loop pieces in anti-diagonal form (tables.py antidiagonal_tables).  With x_n(k) = c_n k^{Pow_n} and
// Pow_n = bias + i dpow (n - 128), the k dependence of a pair (n, m) is k^{2 bias + i dpow (n + m - 256)}: it depends on
// n + m only.  So for every loop matrix M
//     sum_{n,m} x_n M[n,m] x_m = sum_{j'} k^{2 bias + i dpow j'} S[j'],     S[j'] = sum_{n+m=256+j'} c_n c_m M[n,m]
// -- one k-INDEPENDENT pass over the matrix per cosmology (antidiag_kernel: 9 x 33 153 complex MACs) and a 513-term real
// synthesis per output point (synth_kernel on the FP64 matrix cores), instead of 257^2 terms per point
// (reference pybird.py:1074-1078 makeP22, :1103-1125 makeC22 / makeC13).  The same S serve P22 at all k and, multiplied
// by the Bessel weights Ml(n + m), C22 / C13 at all s and l.  The single sums (P13, C11, Cct) are 257-term syntheses.
//   antidiag_kernel    S[w][c][j'], j' = 0..256 (S[-j'] = conj S[j']) for the 7 + 2 basis matrices: wave <-> (j', 64 cosmologies)
//   build_rows_kernel  real coefficient rows (Re Z_0, Re Z_1, Im Z_1, ...): S_c (P22), Ml[l] S_c (C22 / C13), c_n V_n (single sums)
//   synth_kernel       out[row][x] = sum_q rows[row][q] Tab[q][x]   (Tab = x^{..}{1, 2cos, -/+2sin}: tables.py synthesis_table)
//   expand_kernel      the 28 / 10 loop matrices per l from the synthesised basis rows
// ------------------------------------------------------------------------------------------------
constexpr int AD_T = NHALF + 2;   // anti-diagonal length (129) rounded up to even
constexpr int AD_CH = 1;          // partial sums per anti-diagonal in HBM (round 2 cut it into 3 chunks of 44 pairs, summed by build_rows_kernel; round 3 sums inside the workgroup)
constexpr int KSYN = 528;         // 1 + 2*256 synthesis coefficients, zero padded to a multiple of SYN_KPAD
constexpr int KLIN = 288;         // 1 + 2*128, likewise
constexpr int SYN_KPAD = 48;      // every K of a synthesis / first-stage GEMM is zero padded to a multiple of this
constexpr int SYN_KC = 24;        // K chunk of synth_kernel staged in LDS (divides SYN_KPAD); 24 rather than 48: 94 instead of 104 registers per
                                  // lane, which is what fits beside two resummation waves on a SIMD (512 - 2 x 208 = 96)
static_assert(SYN_KPAD % SYN_KC == 0 && (32 * SYN_KC) % 256 == 0, "chunk must divide the padding and fill the staging threads");
constexpr int BAS22 = 8, BASC = 32;  // padded basis rows per cosmology: 7 M22 matrices; Nl * (7 + 2) weighted ones

// Lanes <-> cosmologies (transposed coefficients coefT[2][129][Bmax] come out of the first-stage GEMMs); the matrix weights are wave-uniform
// (scalar loads), so the table is streamed once per 64 cosmologies and no cross-lane reduction is needed.
__device__ __forceinline__ double readlane_f64(double v, int lane) {  // lane: a compile-time constant after unrolling -> two v_readlane_b32 into an SGPR pair
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Round 3.  PMC of the round-2 kernel (one wave per (j', 64 cosmologies, third of the anti-diagonal)): the waves ISSUE half of their
// lifetime and wait a quarter of it -- not latency- but balance-bound: 1 542 waves of 0..44 trips on 1 024 SIMDs, a SIMD that draws two long
// ones sets the launch time (26-28 us for 6 us of issue).  Now a workgroup = 4 waves = one (j', 64 cosmologies): the waves split the anti-diagonal
// evenly, their partial sums meet in LDS in a fixed order (no partial sums in HBM any more: AD_CH = 1), and odd cosmology groups walk j'
// backwards, so that workgroup i and workgroup 257 + i -- which the dispatcher deals to the same CU -- bring 129 - i/2 and 1 + i/2 pairs:
// every CU gets the same work.  Inside a wave:
//   * the weights of PB = 3 consecutive pairs (54 doubles, contiguous in the table) arrive as ONE coalesced wave-load a block ahead and are
//     handed to the FMAs through v_readlane (SGPR operands as before, but no scalar-memory round trip and no "wait for all scalar loads");
//   * the coefficients sit in a ring of PB slots: a slot is reloaded with the pair PB trips ahead as soon as its pair has been consumed.
template <int NC, int NW>
__global__ __launch_bounds__(64 * NW) void antidiag_kernel(int B, int Bmax, const double* __restrict__ coefT,
                                                           const double2* __restrict__ AD, double2* __restrict__ S) {
    constexpr int PB = 3, WPP = 2 * NC;  // pairs per weight block, doubles per pair
    static_assert(PB * WPP <= 64, "one wave-load must hold a block's weights");
    __shared__ double red[NW - 1][2 * NC][64];  // partial sums of waves 1..NW-1
    const int grp = blockIdx.y, jp = (grp & 1) ? NPOW - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w = grp * 64 + lane;
    const int wl = w < B ? w : B - 1;
    const int cnt = ((2 * NHALF + jp) >> 1) - jp + 1;  // pairs (n, m) = (jp + t, 256 - t), n <= m
    const int per = (cnt + NW - 1) / NW, t0 = wave * per, t1 = min(cnt, t0 + per);
    const double* cr = coefT + wl;
    const double* ci = coefT + (size_t)NCH * Bmax + wl;
    double ar[NC], ai[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) ar[q] = ai[q] = 0.0;
    if (t0 < t1) {
        const double* adw = reinterpret_cast<const double*>(AD + ((size_t)jp * AD_T + t0) * NC);  // weights of pair t0 + i: adw[i WPP .. (i + 1) WPP)
        const int nw = (t1 - t0) * WPP;
        auto wload = [&](int blk) { return adw[min(blk * PB * WPP + lane, nw - 1)]; };
        // (loads only -- the conjugations c_{256-n} = conj(c_n), c_m = conj(c_t) for m = 256 - t are applied where the values are consumed)
        double xr[PB], xi[PB], yr[PB], yi[PB];
        auto coef = [&](int t, int p) {
            const int n = jp + t, qn = n <= NHALF ? n : 2 * NHALF - n;
            xr[p] = cr[(size_t)qn * Bmax];
            xi[p] = ci[(size_t)qn * Bmax];
            yr[p] = cr[(size_t)t * Bmax];
            yi[p] = ci[(size_t)t * Bmax];
        };
        double wc = wload(0);
#pragma unroll
        for (int p = 0; p < PB; ++p) coef(min(t0 + p, t1 - 1), p);
        const int nblk = (t1 - t0 + PB - 1) / PB;
        for (int blk = 0; blk < nblk; ++blk) {
            const double wn = wload(blk + 1);  // (clamped to the chunk's last weight: the block after the last one is never consumed)
#pragma unroll
            for (int p = 0; p < PB; ++p) {
                const int t = t0 + blk * PB + p;
                const double on = t < t1 ? 1.0 : 0.0;  // pairs past the chunk's end (the last block's padding) carry no weight
                const double xim = jp + t <= NHALF ? xi[p] : -xi[p], yim = -yi[p];
                const double pr = (xr[p] * yr[p] - xim * yim) * on, pi = (xr[p] * yim + xim * yr[p]) * on;
                // (scheduling barriers: left alone, the compiler gathers the reloads of all slots at the top of the trip and waits for every
                // outstanding load before the first FMA -- no load would be in flight under the arithmetic)
                __builtin_amdgcn_sched_barrier(0);
                coef(min(t + PB, t1 - 1), p);  // the slot has been consumed: its next occupant is requested before this pair's FMAs
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    const double mx = readlane_f64(wc, p * WPP + 2 * q), my = readlane_f64(wc, p * WPP + 2 * q + 1);
                    ar[q] = fma(mx, pr, fma(-my, pi, ar[q]));
                    ai[q] = fma(mx, pi, fma(my, pr, ai[q]));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            wc = wn;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            red[wave - 1][2 * q][lane] = ar[q];
            red[wave - 1][2 * q + 1][lane] = ai[q];
        }
    }
    __syncthreads();
    if (wave == 0 && w < B) {
#pragma unroll
        for (int q = 0; q < NC; ++q) {
#pragma unroll
            for (int v = 0; v < NW - 1; ++v) {  // fixed order: wave 0 + wave 1 + ...
                ar[q] += red[v][2 * q][lane];
                ai[q] += red[v][2 * q + 1][lane];
            }
            S[((size_t)w * NC + q) * NPOW + jp] = make_double2(ar[q], ai[q]);
        }
    }
}

// Any other NFFT = 2 nh (128 <= nh <= 256): the same pass with nh read at run time -- a kernel of its own, so that the NFFT = 256 build above
// keeps its code.  Grid: NPOW = 2 nh + 1 anti-diagonals; the odd cosmology groups walk j' backwards as above, so workgroups i and NPOW + i,
// which the dispatcher deals to the same CU, bring nh + 1 - i/2 and 1 + i/2 pairs between them.
template <int NC, int NW>
__global__ __launch_bounds__(64 * NW) void antidiag_nh_kernel(int B, int Bmax, const double* __restrict__ coefT,
                                                              const double2* __restrict__ AD, double2* __restrict__ S, int nh) {
    constexpr int PB = 3, WPP = 2 * NC;  // pairs per weight block, doubles per pair
    static_assert(PB * WPP <= 64, "one wave-load must hold a block's weights");
    __shared__ double red[NW - 1][2 * NC][64];  // partial sums of waves 1..NW-1
    const int npow = 2 * nh + 1, nch = nh + 1, adt = nh + 2;
    const int grp = blockIdx.y, jp = (grp & 1) ? npow - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w = grp * 64 + lane;
    const int wl = w < B ? w : B - 1;
    const int cnt = ((2 * nh + jp) >> 1) - jp + 1;  // pairs (n, m) = (jp + t, 2 nh - t), n <= m
    const int per = (cnt + NW - 1) / NW, t0 = wave * per, t1 = min(cnt, t0 + per);
    const double* cr = coefT + wl;
    const double* ci = coefT + (size_t)nch * Bmax + wl;
    double ar[NC], ai[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) ar[q] = ai[q] = 0.0;
    if (t0 < t1) {
        const double* adw = reinterpret_cast<const double*>(AD + ((size_t)jp * adt + t0) * NC);  // weights of pair t0 + i: adw[i WPP .. (i + 1) WPP)
        const int nw = (t1 - t0) * WPP;
        auto wload = [&](int blk) { return adw[min(blk * PB * WPP + lane, nw - 1)]; };
        // (loads only -- the conjugations c_{2nh-n} = conj(c_n), c_m = conj(c_t) for m = 2 nh - t are applied where the values are consumed)
        double xr[PB], xi[PB], yr[PB], yi[PB];
        auto coef = [&](int t, int p) {
            const int n = jp + t, qn = n <= nh ? n : 2 * nh - n;
            xr[p] = cr[(size_t)qn * Bmax];
            xi[p] = ci[(size_t)qn * Bmax];
            yr[p] = cr[(size_t)t * Bmax];
            yi[p] = ci[(size_t)t * Bmax];
        };
        double wc = wload(0);
#pragma unroll
        for (int p = 0; p < PB; ++p) coef(min(t0 + p, t1 - 1), p);
        const int nblk = (t1 - t0 + PB - 1) / PB;
        for (int blk = 0; blk < nblk; ++blk) {
            const double wn = wload(blk + 1);  // (clamped to the chunk's last weight: the block after the last one is never consumed)
#pragma unroll
            for (int p = 0; p < PB; ++p) {
                const int t = t0 + blk * PB + p;
                const double on = t < t1 ? 1.0 : 0.0;  // pairs past the chunk's end (the last block's padding) carry no weight
                const double xim = jp + t <= nh ? xi[p] : -xi[p], yim = -yi[p];
                const double pr = (xr[p] * yr[p] - xim * yim) * on, pi = (xr[p] * yim + xim * yr[p]) * on;
                // (scheduling barriers: left alone, the compiler gathers the reloads of all slots at the top of the trip and waits for every
                // outstanding load before the first FMA -- no load would be in flight under the arithmetic)
                __builtin_amdgcn_sched_barrier(0);
                coef(min(t + PB, t1 - 1), p);  // the slot has been consumed: its next occupant is requested before this pair's FMAs
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    const double mx = readlane_f64(wc, p * WPP + 2 * q), my = readlane_f64(wc, p * WPP + 2 * q + 1);
                    ar[q] = fma(mx, pr, fma(-my, pi, ar[q]));
                    ai[q] = fma(mx, pi, fma(my, pr, ai[q]));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            wc = wn;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            red[wave - 1][2 * q][lane] = ar[q];
            red[wave - 1][2 * q + 1][lane] = ai[q];
        }
    }
    __syncthreads();
    if (wave == 0 && w < B) {
#pragma unroll
        for (int q = 0; q < NC; ++q) {
#pragma unroll
            for (int v = 0; v < NW - 1; ++v) {  // fixed order: wave 0 + wave 1 + ...
                ar[q] += red[v][2 * q][lane];
                ai[q] += red[v][2 * q + 1][lane];
            }
            S[((size_t)w * NC + q) * npow + jp] = make_double2(ar[q], ai[q]);
        }
    }
}

// One lane = one j' of one cosmology: sums the AD_CH partials of the nc anti-diagonal sums once, then writes
//   blockIdx.y = 0: the nb P22 basis rows  (A22[w][BAS22][KSYN])  and the 10 P13 rows (A13[w][10][KLIN])
//   blockIdx.y = 1: the Nl*nc weighted rows Ml[l] S_c (ACF[w][BASC][KSYN]) and the nlc Nl C11 / Cct (/ CctNNLO) rows (ALC[w][nlc Nl][KLIN])
// as real synthesis coefficients (Re Z_0, Re Z_1, Im Z_1, ...).  `sets` bit 0/1: quadratic rows of y = 0/1, bit 2/3: linear rows.
template <int NC>
__global__ __launch_bounds__(64) void build_rows_kernel(int sets, int Bmax, int Nl, int nlc, int nb, const double* __restrict__ coef,
                                                         const double2* __restrict__ S, const double2* __restrict__ mlj,
                                                         const double2* __restrict__ linvec, double* __restrict__ A22,
                                                         double* __restrict__ A13, double* __restrict__ ACF, double* __restrict__ ALC) {
    // five single-wave workgroups per (cosmology, half) for the 257 harmonics (round 3: as ONE workgroup of 320 threads the kernel took 58 us
    // beside the resummation against 9 alone -- five waves need two free wave slots on one SIMD, which two resummation waves never leave)
    const int w = blockIdx.x, cf = blockIdx.y, jp = blockIdx.z * 64 + threadIdx.x;
    if (((sets >> cf) & 1) && jp < NPOW) {
        double zr[NC], zi[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            zr[q] = zi[q] = 0.0;
#pragma unroll
            for (int ch = 0; ch < AD_CH; ++ch) {
                const double2 v = S[(((size_t)ch * Bmax + w) * NC + q) * NPOW + jp];
                zr[q] += v.x;
                zi[q] += v.y;
            }
        }
        const int o0 = jp == 0 ? 0 : 2 * jp - 1;
        if (cf == 0) {
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (q < nb) {
                    double* o = A22 + ((size_t)w * BAS22 + q) * KSYN;
                    o[o0] = zr[q];
                    if (jp) o[o0 + 1] = zi[q];
                }
        } else {
            for (int l = 0; l < Nl; ++l) {
                const double2 m = mlj[l * NPOW + jp];  // Bessel weight Ml[l](n + m) (reference pybird.py:1040-1046)
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    double* o = ACF + ((size_t)w * BASC + l * NC + q) * KSYN;
                    o[o0] = m.x * zr[q] - m.y * zi[q];
                    if (jp) o[o0 + 1] = m.x * zi[q] + m.y * zr[q];
                }
            }
        }
    }
    if ((sets >> (2 + cf)) & 1) {
        const int nrows = cf == 0 ? 10 : nlc * Nl, v0 = cf == 0 ? 0 : 10;  // nlc = 2 (C11, Cct) or 3 (+ CctNNLO)
        double* out = cf == 0 ? A13 + (size_t)w * 10 * KLIN : ALC + (size_t)w * nlc * Nl * KLIN;
        const double* c = coef + (size_t)w * 2 * NCH;
        for (int e = jp; e < nrows * NCH; e += 320) {
            const int row = e / NCH, mp = e % NCH, n = NHALF - mp;  // harmonic mp <-> coefficient n = 128 - mp
            const double2 v = linvec[(size_t)(v0 + row) * NCH + n];
            const double cr = c[n], ci = n == NHALF ? 0.0 : c[NCH + n];
            double* o = out + (size_t)row * KLIN;
            if (mp == 0) o[0] = cr * v.x - ci * v.y;
            else {
                o[2 * mp - 1] = cr * v.x - ci * v.y;
                o[2 * mp] = cr * v.y + ci * v.x;
            }
        }
    }
}

// Row lengths of the loop syntheses for NFFT = 2 nh: 1 + 4 nh (double sums) and 1 + 2 nh (single sums), zero padded to SYN_KPAD
__host__ __device__ constexpr int ksyn_of(int nh) { return (4 * nh + SYN_KPAD) / SYN_KPAD * SYN_KPAD; }
__host__ __device__ constexpr int klin_of(int nh) { return (2 * nh + SYN_KPAD) / SYN_KPAD * SYN_KPAD; }
static_assert(ksyn_of(NHALF) == KSYN && klin_of(NHALF) == KLIN, "row lengths of the default NFFT");

template <int NC>
__global__ __launch_bounds__(64) void build_rows_nh_kernel(int sets, int Bmax, int Nl, int nlc, int nb, const double* __restrict__ coef,
                                                            const double2* __restrict__ S, const double2* __restrict__ mlj,
                                                            const double2* __restrict__ linvec, double* __restrict__ A22,
                                                            double* __restrict__ A13, double* __restrict__ ACF, double* __restrict__ ALC, int nh) {
    // five single-wave workgroups per (cosmology, half) for the 257 harmonics (round 3: as ONE workgroup of 320 threads the kernel took 58 us
    // beside the resummation against 9 alone -- five waves need two free wave slots on one SIMD, which two resummation waves never leave);
    // ceil((2 nh + 1) / 64) of them at other NFFT
    const int npow = 2 * nh + 1, nch = nh + 1, ksyn = ksyn_of(nh), klin = klin_of(nh), zstride = 64 * (int)gridDim.z;
    const int w = blockIdx.x, cf = blockIdx.y, jp = blockIdx.z * 64 + threadIdx.x;
    if (((sets >> cf) & 1) && jp < npow) {
        double zr[NC], zi[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            zr[q] = zi[q] = 0.0;
#pragma unroll
            for (int ch = 0; ch < AD_CH; ++ch) {
                const double2 v = S[(((size_t)ch * Bmax + w) * NC + q) * npow + jp];
                zr[q] += v.x;
                zi[q] += v.y;
            }
        }
        const int o0 = jp == 0 ? 0 : 2 * jp - 1;
        if (cf == 0) {
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (q < nb) {
                    double* o = A22 + ((size_t)w * BAS22 + q) * ksyn;
                    o[o0] = zr[q];
                    if (jp) o[o0 + 1] = zi[q];
                }
        } else {
            for (int l = 0; l < Nl; ++l) {
                const double2 m = mlj[l * npow + jp];  // Bessel weight Ml[l](n + m) (reference pybird.py:1040-1046)
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    double* o = ACF + ((size_t)w * BASC + l * NC + q) * ksyn;
                    o[o0] = m.x * zr[q] - m.y * zi[q];
                    if (jp) o[o0 + 1] = m.x * zi[q] + m.y * zr[q];
                }
            }
        }
    }
    if ((sets >> (2 + cf)) & 1) {
        const int nrows = cf == 0 ? 10 : nlc * Nl, v0 = cf == 0 ? 0 : 10;  // nlc = 2 (C11, Cct) or 3 (+ CctNNLO)
        double* out = cf == 0 ? A13 + (size_t)w * 10 * klin : ALC + (size_t)w * nlc * Nl * klin;
        const double* c = coef + (size_t)w * 2 * nch;
        for (int e = jp; e < nrows * nch; e += zstride) {
            const int row = e / nch, mp = e % nch, n = nh - mp;  // harmonic mp <-> coefficient n = nh - mp
            const double2 v = linvec[(size_t)(v0 + row) * nch + n];
            const double cr = c[n], ci = n == nh ? 0.0 : c[nch + n];
            double* o = out + (size_t)row * klin;
            if (mp == 0) o[0] = cr * v.x - ci * v.y;
            else {
                o[2 * mp - 1] = cr * v.x - ci * v.y;
                o[2 * mp] = cr * v.y + ci * v.x;
            }
        }
    }
}

__device__ inline double ipow(double f, int p) {
    double r = 1.0;
    for (int i = 0; i < p; ++i) r *= f;
    return r;
}

// Direct-P_l runs (EFTB_O_PLK_DIRECT): the bias contraction commutes with the synthesis as well -- it is linear in the rows -- so the rows are
// contracted HERE, before the matrix-core products: per cosmology 3 rows (one per multipole) instead of 7 for the P22 basis, 3 instead of 10 for
// P13, 3 instead of Nl (7 + 2) = 27 for the xi-space basis; the C11 / Cct rows are scaled by sum_i b_i l11[l'][i] / sum_i b_3+i lct[l'][i].
// Weights: cf_l[b] = b_group(b) f^power(b) mu-weight_l(b) per loop piece b (regroup_kernel), contracted with the combination matrices of the
// loop-matrix basis (tables.loop_basis: exp22 [28][BAS22], expc [Nl 38][BASC], block-diagonal in l).  Same grid and lanes as build_rows_kernel.
template <int NC>
__global__ __launch_bounds__(64) void build_rows_plk_kernel(int Bmax, int nb, const double* __restrict__ coef, const double2* __restrict__ S,
                                                             const double2* __restrict__ mlj, const double2* __restrict__ linvec,
                                                             const double* __restrict__ bias, const double* __restrict__ fgrow,
                                                             const double* __restrict__ l11, const double* __restrict__ lct,
                                                             const double* __restrict__ l22, const double* __restrict__ l13,
                                                             const int* __restrict__ grp, const double* __restrict__ exp22,
                                                             const double* __restrict__ expc, double* __restrict__ A22, double* __restrict__ A13,
                                                             double* __restrict__ ACF, double* __restrict__ ALC) {
    constexpr int NL = 3;
    __shared__ double s_cf[NL * 38];   // cf_l[b]
    __shared__ double s_w[NL * NC];    // k space: sum_b cf_l[b] exp22[b][q] (q < nb); xi space: sum_b cf_l'[b] expc[row(l', b)][l' NC + q]
    __shared__ double s_b[2 * NL];
    const int w = blockIdx.x, cf = blockIdx.y, jp = blockIdx.z * 64 + threadIdx.x;
    const double* bw = bias + (size_t)w * NROW;
    const double f = fgrow[w];
    for (int e = threadIdx.x; e < NL * 38; e += 64) {
        const int l = e / 38, bq = e % 38;
        s_cf[e] = bw[9 + grp[2 * bq]] * ipow(f, grp[2 * bq + 1]) * (bq < 28 ? l22[l * 28 + bq] : l13[l * 10 + (bq - 28)]);
    }
    if (threadIdx.x < 2 * NL) {
        const int a = threadIdx.x / NL, lp = threadIdx.x % NL;
        double v = 0.0;
        if (a == 0)
            for (int r = 0; r < 3; ++r) v = fma(bw[r], l11[lp * 3 + r], v);
        else
            for (int r = 0; r < 6; ++r) v = fma(bw[3 + r], lct[lp * 6 + r], v);
        s_b[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x < NL * NC) {
        const int l = threadIdx.x / NC, q = threadIdx.x % NC;
        double v0 = 0.0, v1 = 0.0;
        if (cf == 0) {
            if (q < nb)
                for (int b = 0; b < 28; b += 2) {
                    v0 = fma(s_cf[l * 38 + b], exp22[b * BAS22 + q], v0);
                    v1 = fma(s_cf[l * 38 + b + 1], exp22[(b + 1) * BAS22 + q], v1);
                }
        } else {
            for (int b = 0; b < 28; b += 2) {
                v0 = fma(s_cf[l * 38 + b], expc[(size_t)(l * 28 + b) * BASC + l * NC + q], v0);
                v1 = fma(s_cf[l * 38 + b + 1], expc[(size_t)(l * 28 + b + 1) * BASC + l * NC + q], v1);
            }
            for (int b = 0; b < 10; b += 2) {
                v0 = fma(s_cf[l * 38 + 28 + b], expc[(size_t)(NL * 28 + l * 10 + b) * BASC + l * NC + q], v0);
                v1 = fma(s_cf[l * 38 + 29 + b], expc[(size_t)(NL * 28 + l * 10 + b + 1) * BASC + l * NC + q], v1);
            }
        }
        s_w[threadIdx.x] = v0 + v1;
    }
    __syncthreads();
    if (jp < NPOW) {
        double zr[NC], zi[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            zr[q] = zi[q] = 0.0;
#pragma unroll
            for (int ch = 0; ch < AD_CH; ++ch) {
                const double2 v = S[(((size_t)ch * Bmax + w) * NC + q) * NPOW + jp];
                zr[q] += v.x;
                zi[q] += v.y;
            }
        }
        const int o0 = jp == 0 ? 0 : 2 * jp - 1;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            double cr = 0.0, ci = 0.0;
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                cr = fma(s_w[l * NC + q], zr[q], cr);
                ci = fma(s_w[l * NC + q], zi[q], ci);
            }
            if (cf == 0) {
                double* o = A22 + ((size_t)w * BAS22 + l) * KSYN;
                o[o0] = cr;
                if (jp) o[o0 + 1] = ci;
            } else {
                const double2 m = mlj[l * NPOW + jp];  // Bessel weight Ml[l](n + m) (reference pybird.py:1040-1046)
                double* o = ACF + ((size_t)w * BASC + l) * KSYN;
                o[o0] = m.x * cr - m.y * ci;
                if (jp) o[o0 + 1] = m.x * ci + m.y * cr;
            }
        }
    }
    {   // single-sum rows: k space -> the 10 P13 rows contracted with cf_l[28 + b] (3 rows); xi space -> C11[l'] x s_b[l'], Cct[l'] x s_b[NL + l']
        const int nrows = cf == 0 ? NL : 2 * NL;
        double* out = cf == 0 ? A13 + (size_t)w * 10 * KLIN : ALC + (size_t)w * 2 * NL * KLIN;
        const double* c = coef + (size_t)w * 2 * NCH;
        for (int e = jp; e < nrows * NCH; e += 320) {
            const int row = e / NCH, mp = e % NCH, n = NHALF - mp;  // harmonic mp <-> coefficient n = 128 - mp
            double vx, vy;
            if (cf == 0) {
                vx = vy = 0.0;
#pragma unroll
                for (int b = 0; b < 10; ++b) {
                    const double2 v = linvec[(size_t)b * NCH + n];
                    vx = fma(s_cf[row * 38 + 28 + b], v.x, vx);
                    vy = fma(s_cf[row * 38 + 28 + b], v.y, vy);
                }
            } else {
                const double2 v = linvec[(size_t)(10 + row) * NCH + n];
                vx = s_b[row] * v.x;
                vy = s_b[row] * v.y;
            }
            const double cr = c[n], ci = n == NHALF ? 0.0 : c[NCH + n];
            double* o = out + (size_t)row * KLIN;
            if (mp == 0) o[0] = cr * vx - ci * vy;
            else {
                o[2 * mp - 1] = cr * vx - ci * vy;
                o[2 * mp] = cr * vy + ci * vx;
            }
        }
    }
}

// build_rows_plk_kernel at any other NFFT = 2 nh (nh read at run time; ceil((2 nh + 1) / 64) workgroups per (cosmology, half))
template <int NC>
__global__ __launch_bounds__(64) void build_rows_plk_nh_kernel(int Bmax, int nb, const double* __restrict__ coef, const double2* __restrict__ S,
                                                    const double2* __restrict__ mlj, const double2* __restrict__ linvec,
                                                    const double* __restrict__ bias, const double* __restrict__ fgrow,
                                                    const double* __restrict__ l11, const double* __restrict__ lct,
                                                    const double* __restrict__ l22, const double* __restrict__ l13,
                                                    const int* __restrict__ grp, const double* __restrict__ exp22,
                                                    const double* __restrict__ expc, double* __restrict__ A22, double* __restrict__ A13,
                                                    double* __restrict__ ACF, double* __restrict__ ALC, int nh) {
    constexpr int NL = 3;
    const int npow = 2 * nh + 1, nch = nh + 1, ksyn = ksyn_of(nh), klin = klin_of(nh), zstride = 64 * (int)gridDim.z;
    __shared__ double s_cf[NL * 38];   // cf_l[b]
    __shared__ double s_w[NL * NC];    // k space: sum_b cf_l[b] exp22[b][q] (q < nb); xi space: sum_b cf_l'[b] expc[row(l', b)][l' NC + q]
    __shared__ double s_b[2 * NL];
    const int w = blockIdx.x, cf = blockIdx.y, jp = blockIdx.z * 64 + threadIdx.x;
    const double* bw = bias + (size_t)w * NROW;
    const double f = fgrow[w];
    for (int e = threadIdx.x; e < NL * 38; e += 64) {
        const int l = e / 38, bq = e % 38;
        s_cf[e] = bw[9 + grp[2 * bq]] * ipow(f, grp[2 * bq + 1]) * (bq < 28 ? l22[l * 28 + bq] : l13[l * 10 + (bq - 28)]);
    }
    if (threadIdx.x < 2 * NL) {
        const int a = threadIdx.x / NL, lp = threadIdx.x % NL;
        double v = 0.0;
        if (a == 0)
            for (int r = 0; r < 3; ++r) v = fma(bw[r], l11[lp * 3 + r], v);
        else
            for (int r = 0; r < 6; ++r) v = fma(bw[3 + r], lct[lp * 6 + r], v);
        s_b[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x < NL * NC) {
        const int l = threadIdx.x / NC, q = threadIdx.x % NC;
        double v0 = 0.0, v1 = 0.0;
        if (cf == 0) {
            if (q < nb)
                for (int b = 0; b < 28; b += 2) {
                    v0 = fma(s_cf[l * 38 + b], exp22[b * BAS22 + q], v0);
                    v1 = fma(s_cf[l * 38 + b + 1], exp22[(b + 1) * BAS22 + q], v1);
                }
        } else {
            for (int b = 0; b < 28; b += 2) {
                v0 = fma(s_cf[l * 38 + b], expc[(size_t)(l * 28 + b) * BASC + l * NC + q], v0);
                v1 = fma(s_cf[l * 38 + b + 1], expc[(size_t)(l * 28 + b + 1) * BASC + l * NC + q], v1);
            }
            for (int b = 0; b < 10; b += 2) {
                v0 = fma(s_cf[l * 38 + 28 + b], expc[(size_t)(NL * 28 + l * 10 + b) * BASC + l * NC + q], v0);
                v1 = fma(s_cf[l * 38 + 29 + b], expc[(size_t)(NL * 28 + l * 10 + b + 1) * BASC + l * NC + q], v1);
            }
        }
        s_w[threadIdx.x] = v0 + v1;
    }
    __syncthreads();
    if (jp < npow) {
        double zr[NC], zi[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            zr[q] = zi[q] = 0.0;
#pragma unroll
            for (int ch = 0; ch < AD_CH; ++ch) {
                const double2 v = S[(((size_t)ch * Bmax + w) * NC + q) * npow + jp];
                zr[q] += v.x;
                zi[q] += v.y;
            }
        }
        const int o0 = jp == 0 ? 0 : 2 * jp - 1;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            double cr = 0.0, ci = 0.0;
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                cr = fma(s_w[l * NC + q], zr[q], cr);
                ci = fma(s_w[l * NC + q], zi[q], ci);
            }
            if (cf == 0) {
                double* o = A22 + ((size_t)w * BAS22 + l) * ksyn;
                o[o0] = cr;
                if (jp) o[o0 + 1] = ci;
            } else {
                const double2 m = mlj[l * npow + jp];  // Bessel weight Ml[l](n + m) (reference pybird.py:1040-1046)
                double* o = ACF + ((size_t)w * BASC + l) * ksyn;
                o[o0] = m.x * cr - m.y * ci;
                if (jp) o[o0 + 1] = m.x * ci + m.y * cr;
            }
        }
    }
    {   // single-sum rows: k space -> the 10 P13 rows contracted with cf_l[28 + b] (3 rows); xi space -> C11[l'] x s_b[l'], Cct[l'] x s_b[NL + l']
        const int nrows = cf == 0 ? NL : 2 * NL;
        double* out = cf == 0 ? A13 + (size_t)w * 10 * klin : ALC + (size_t)w * 2 * NL * klin;
        const double* c = coef + (size_t)w * 2 * nch;
        for (int e = jp; e < nrows * nch; e += zstride) {
            const int row = e / nch, mp = e % nch, n = nh - mp;  // harmonic mp <-> coefficient n = nh - mp
            double vx, vy;
            if (cf == 0) {
                vx = vy = 0.0;
#pragma unroll
                for (int b = 0; b < 10; ++b) {
                    const double2 v = linvec[(size_t)b * nch + n];
                    vx = fma(s_cf[row * 38 + 28 + b], v.x, vx);
                    vy = fma(s_cf[row * 38 + 28 + b], v.y, vy);
                }
            } else {
                const double2 v = linvec[(size_t)(10 + row) * nch + n];
                vx = s_b[row] * v.x;
                vy = s_b[row] * v.y;
            }
            const double cr = c[n], ci = n == nh ? 0.0 : c[nch + n];
            double* o = out + (size_t)row * klin;
            if (mp == 0) o[0] = cr * vx - ci * vy;
            else {
                o[2 * mp - 1] = cr * vx - ci * vy;
                o[2 * mp] = cr * vy + ci * vx;
            }
        }
    }
}

// out[row][x] = sum_q A[row][q] Tab[q][x]  (* gscale[row / rpg][x]) (* xscale[x]) on the FP64 matrix cores.  Rows are
// addressed as (group = row / rpg, member = row % rpg): A + group a_group + member K, out + group o_group + member X.
// Workgroup = 4 waves = 32 rows x 64 x; A and Tab chunks of SYN_KC go through LDS (strides 50 / 80: conflict-free
// ds_read_b64 for the MFMA operand layouts), each wave owns 16 rows x 32 x.
struct SynthDesc {
    const double* A;
    const double* Tab;    // [K][X]
    double* out;
    const double* gscale; // [groups][X] or null   (P13: P11)
    const double* xscale; // [X] or null           (Cct: s^-2)
    long long a_group, o_group;
    int M, rpg, K, X;
    int wg_end, wgx;      // batched launch: this problem owns workgroups [previous wg_end, wg_end), wgx of them per row tile
};

// Several independent syntheses in one launch (P22 basis, P13, xi basis, C11, Cct): each is latency-bound on its own
// (a few hundred workgroups, a global-load round trip per K chunk), together they fill the chip.
constexpr int SYN_MAXP = 6;
struct SynthBatch {
    SynthDesc p[SYN_MAXP];
    int n;
};

__global__ __launch_bounds__(256) void synth_kernel(SynthBatch batch) {
    int pi = 0, wg0 = 0;
#pragma unroll
    for (int q = 0; q < SYN_MAXP - 1; ++q)
        if (q + 1 < batch.n && (int)blockIdx.x >= batch.p[q].wg_end) {
            pi = q + 1;
            wg0 = batch.p[q].wg_end;
        }
    const SynthDesc& d = batch.p[pi];
    const int wg = blockIdx.x - wg0, bx = wg % d.wgx, by = wg / d.wgx;
    constexpr int LDA = SYN_KC + 2, LDB = 80, NA = 32 * SYN_KC / 256, NB = SYN_KC * 64 / 256;
    __shared__ double As[32 * LDA];
    __shared__ double Bs[SYN_KC * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int row0 = by * 32, x0 = bx * 64;
    const int rh = wave >> 1, xh = wave & 1;
    // this thread's share of every chunk: NA elements of the A tile, NB of the Tab tile at fixed positions.  Kept as 32-bit element
    // offsets and bit masks (not pointers and multipliers): the kernel must fit beside two waves of the resummation kernel on a SIMD,
    // i.e. in ~100 VGPRs, or its workgroups wait for a whole resummation wave to retire before they can start
    int offa[NA];       // element offset of A[row][kk] from d.A (chunk 0)
    unsigned amask = 0; // bit i: row of element i is inside the problem
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int e = tid + 256 * i, rr = e / SYN_KC, kk = e % SYN_KC, row = row0 + rr, rc = row < d.M ? row : d.M - 1;
        offa[i] = (int)((long long)(rc / d.rpg) * d.a_group + (long long)(rc % d.rpg) * d.K + kk);
        amask |= (row < d.M ? 1u : 0u) << i;
    }
    const int kb = tid >> 6, xx = tid & 63;  // Tab element i sits at row kb + 4 i of the chunk, column x0 + xx
    const bool xlive = x0 + xx < d.X;
    const double* tb0 = d.Tab + (size_t)kb * d.X + (xlive ? x0 + xx : d.X - 1);
    const size_t tstep = (size_t)4 * d.X;
    double va[NA], vb[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) va[i] = d.A[offa[i]];
#pragma unroll
    for (int i = 0; i < NB; ++i) vb[i] = tb0[i * tstep];
    v4d acc[2] = {(v4d){0.0, 0.0, 0.0, 0.0}, (v4d){0.0, 0.0, 0.0, 0.0}};
    const int xw = x0 + xh * 32, ncol = xw + 16 < d.X ? 2 : (xw < d.X ? 1 : 0);  // this wave's column tiles inside the problem
    for (int k0 = 0; k0 < d.K; k0 += SYN_KC) {
        __syncthreads();  // the previous chunk has been consumed
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = tid + 256 * i;
            As[(e / SYN_KC) * LDA + e % SYN_KC] = (amask >> i) & 1u ? va[i] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) Bs[(kb + 4 * i) * LDB + xx] = xlive ? vb[i] : 0.0;
        __syncthreads();
        if (k0 + SYN_KC < d.K) {  // next chunk's global loads fly under this chunk's MFMAs
            const double* an = d.A + k0 + SYN_KC;
            const double* tn = tb0 + (size_t)(k0 + SYN_KC) * d.X;
#pragma unroll
            for (int i = 0; i < NA; ++i) va[i] = an[offa[i]];
#pragma unroll
            for (int i = 0; i < NB; ++i) vb[i] = tn[i * tstep];
        }
        // (column tiles that lie wholly past the problem's last column issue nothing: X = 80 fills 5 of the 8 tiles of its two workgroup columns,
        // and the FP64 matrix pipe is what this kernel shares with the resummation -- beside it, its time is its MFMA count)
        if (ncol == 2) {
#pragma unroll 4
            for (int t = 0; t < SYN_KC / 4; ++t) {  // (four k-steps of operands in flight: a full unroll costs 40 more registers)
                const double a = As[(rh * 16 + r) * LDA + 4 * t + g];
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[(4 * t + g) * LDB + xh * 32 + 16 * j + r], acc[j], 0, 0, 0);
            }
        } else if (ncol == 1) {
#pragma unroll 4
            for (int t = 0; t < SYN_KC / 4; ++t)
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(rh * 16 + r) * LDA + 4 * t + g], Bs[(4 * t + g) * LDB + xh * 32 + r], acc[0], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = row0 + rh * 16 + g + 4 * q, x = x0 + xh * 32 + 16 * j + r;
            if (row < d.M && x < d.X) {
                const int grp = row / d.rpg, mem = row % d.rpg;
                double v = acc[j][q];
                if (d.gscale) v *= d.gscale[(size_t)grp * d.X + x];
                if (d.xscale) v *= d.xscale[x];
                d.out[(size_t)grp * d.o_group + (size_t)mem * d.X + x] = v;
            }
        }
}

// The same product for problems with FEW rows (the first stage: M = batch, a few hundred columns, K <= 288): one workgroup = one tile of 16 rows
// x 32 columns, operands straight from global memory into the MFMA lanes -- no LDS staging, no barrier in the K loop, ~96 registers per lane.
// synth_kernel's 32 x 64 tiles give such a problem 20-50 workgroups, each walking K in 24-deep chunks behind two barriers and a global ->
// register -> LDS hop per chunk: 35 us alone and 90 us beside the resummation for 0.08 GFLOP (round-3 trace: the look-ahead chain is the
// critical path of a step, and this was its longest link).
// K runs in groups of 16: lane (r = lane & 15, g = lane >> 4) holds A[row r][16 u + 4 g + j] (one 32-byte load) and multiplies it, for
// j = 0..3, with Tab[16 u + 4 g + j][x0 + 2 r + {0, 1}] (one 16-byte load): the k order inside an MFMA is a permutation of the usual one, the
// same on both operands.  Column tile t holds x0 + 2 r + t, so a lane stores pairs of neighbouring columns.  K is a multiple of 16 (SYN_KPAD).
template <int NW>
__global__ __launch_bounds__(64 * NW) void gemm_direct_kernel(SynthBatch batch) {
    // workgroup = NW waves = ONE tile: the waves take an NW-th of the K groups each (the serial depth of a tile is what a problem this small
    // waits for: 18 dependent load -> MFMA trips at K = 288 become 5 with four waves) and their partial tiles meet in LDS, added in wave order
    __shared__ double red[NW - 1][8][64];
    int pi = 0, wg0 = 0;
#pragma unroll
    for (int q = 0; q < SYN_MAXP - 1; ++q)
        if (q + 1 < batch.n && (int)blockIdx.x >= batch.p[q].wg_end) {
            pi = q + 1;
            wg0 = batch.p[q].wg_end;
        }
    const SynthDesc& d = batch.p[pi];
    const int wg = blockIdx.x - wg0, bx = wg % d.wgx, by = wg / d.wgx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int rowa = by * 16 + r, rc = rowa < d.M ? rowa : d.M - 1;
    const double* ap = d.A + (long long)(rc / d.rpg) * d.a_group + (long long)(rc % d.rpg) * d.K + 4 * g;
    const int x = bx * 32 + 2 * r;
    const bool pairs = !(d.X & 1);  // (16-byte loads of two neighbouring columns need an even row length)
    const int x0 = x < d.X ? x : d.X - 1, x1 = x + 1 < d.X ? x + 1 : d.X - 1;
    const double* bp = d.Tab + (size_t)(4 * g) * d.X;
    v4d acc0 = (v4d){0.0, 0.0, 0.0, 0.0}, acc1 = (v4d){0.0, 0.0, 0.0, 0.0};
    const int ng = d.K / 16, per = (ng + NW - 1) / NW, u0 = wave * per, u1 = min(ng, u0 + per);
    if (pairs) {
        const double* bq = bp + (x + 1 < d.X ? x : d.X - 2);
#pragma unroll 2
        for (int u = u0; u < u1; ++u) {
            const double4 a = *reinterpret_cast<const double4*>(ap + 16 * u);
            double2 b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const double2*>(bq + (size_t)(16 * u + j) * d.X);
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b[0].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b[0].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b[1].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b[1].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.z, b[2].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.z, b[2].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.w, b[3].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.w, b[3].y, acc1, 0, 0, 0);
        }
    } else {
#pragma unroll 2
        for (int u = u0; u < u1; ++u) {
            const double4 a = *reinterpret_cast<const double4*>(ap + 16 * u);
            const double av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double* br = bp + (size_t)(16 * u + j) * d.X;
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[j], br[x0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[j], br[x1], acc1, 0, 0, 0);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            red[wave - 1][q][lane] = acc0[q];
            red[wave - 1][4 + q][lane] = acc1[q];
        }
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int v = 0; v < NW - 1; ++v)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc0[q] += red[v][q][lane];
            acc1[q] += red[v][4 + q][lane];
        }
    // D: rows g + 4 q, column r of each tile -> x and x + 1
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = by * 16 + g + 4 * q;
        if (row < d.M && x < d.X) {
            const int grp = row / d.rpg, mem = row % d.rpg;
            double v0 = acc0[q], v1 = acc1[q];
            if (d.gscale) {
                v0 *= d.gscale[(size_t)grp * d.X + x];
                if (x + 1 < d.X) v1 *= d.gscale[(size_t)grp * d.X + x + 1];
            }
            if (d.xscale) {
                v0 *= d.xscale[x];
                if (x + 1 < d.X) v1 *= d.xscale[x + 1];
            }
            double* o = d.out + (size_t)grp * d.o_group + (size_t)mem * d.X + x;
            if (pairs) *reinterpret_cast<double2*>(o) = make_double2(v0, v1);  // (x even, X even: x + 1 < X)
            else {
                o[0] = v0;
                if (x + 1 < d.X) o[1] = v1;
            }
        }
    }
}

// out[g][r][x] = sum_c comb[r][c] basis[g][c][x]: the 28 (10) loop matrices from their 7 (2) basis matrices
// (tables.py loop_basis); one lane = one x of one cosmology and EXP_RPB output rows, the basis values stay in registers.
constexpr int EXP_RPB = 8;

template <int RIN>
__device__ inline void expand_body(int bx, int grp, int bz, int Rout, int X, const double* __restrict__ basis,
                                   const double* __restrict__ comb, double* __restrict__ out) {
    const int x = bx * 64 + threadIdx.x, r0 = bz * EXP_RPB;
    if (x >= X) return;
    double v[RIN];
#pragma unroll
    for (int c = 0; c < RIN; ++c) v[c] = basis[((size_t)grp * RIN + c) * X + x];
    double acc[EXP_RPB];
#pragma unroll
    for (int i = 0; i < EXP_RPB; ++i) acc[i] = 0.0;
#pragma unroll
    for (int c = 0; c < RIN; ++c)
#pragma unroll
        for (int i = 0; i < EXP_RPB; ++i) acc[i] = fma(comb[(size_t)min(r0 + i, Rout - 1) * RIN + c], v[c], acc[i]);  // comb: wave-uniform
#pragma unroll
    for (int i = 0; i < EXP_RPB; ++i)
        if (r0 + i < Rout) out[((size_t)grp * Rout + r0 + i) * X + x] = acc[i];
}

// both expansions in one launch: workgroups [0, n22) -> P22 (28 rows from BAS22, X = Nk), the rest -> C22 / C13 (Nl*38 rows
// from BASC, X = 80); within a part the index runs (x tile, row block, cosmology), x fastest
__global__ __launch_bounds__(64) void expand_kernel(int n22, int Nk, int B, const double* __restrict__ Y22, const double* __restrict__ exp22,
                                                    double* __restrict__ P22, int RoutC, const double* __restrict__ YCF,
                                                    const double* __restrict__ expc, double* __restrict__ CC) {
    int wg = blockIdx.x;
    if (wg < n22) {
        const int nx = (Nk + 63) / 64, nz = (28 + EXP_RPB - 1) / EXP_RPB;
        expand_body<BAS22>(wg % nx, wg / (nx * nz), (wg / nx) % nz, 28, Nk, Y22, exp22, P22);
    } else {
        wg -= n22;
        const int nx = (NS + 63) / 64, nz = (RoutC + EXP_RPB - 1) / EXP_RPB;
        expand_body<BASC>(wg % nx, wg / (nx * nz), (wg / nx) % nz, RoutC, NS, YCF, expc, CC);
    }
}

// ------------------------------------------------------------------------------------------------
// General FP64-MFMA GEMM for the smaller dense stages:  C[row][col] = sum_seg sum_k A_seg[row][k] B_seg[k][col].
//   * post-AP projection: out[(w,r)][(a,x)] = sum_{l,k} T[w][l][r][k] ProjT[(l,k)][(a,x)]  (window / binning / chained)
// Workgroup = 4 waves = 64 rows x 256 columns; wave q owns column tiles 4q..4q+3 (16 accumulator tiles); the A
// tile (64 rows x <= 256 k) is staged in LDS per K chunk (stride KC+2 -> conflict-free ds_read_b64), B is read
// row-major, 4 x 128 contiguous bytes per fragment.  Row/column addressing is two-level (group, member) so that
// the template block [w][l][r][k] and the output [w][a][r][x] need no repacking.
// ------------------------------------------------------------------------------------------------
struct GemmDesc {
    const double* A; long long a_group, a_row, a_seg; int rows, rows_per_group, nseg, kseg;
    const double* B; int ldb, ncols;
    double* C; long long c_group, c_row, c_colgroup; int cols_per_group;
};

__global__ __launch_bounds__(256, 1) void gemm_rows_kernel(GemmDesc d) {
    constexpr int MT = 4, NT = 4, ROWS = 64, KC = 256, LD = KC + 2;
    extern __shared__ double sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * ROWS, col0 = blockIdx.y * 256 + wave * 64;
    v4d acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    const bool wave_live = col0 < d.ncols;
    for (int seg = 0; seg < d.nseg; ++seg) {
        for (int kc0 = 0; kc0 < d.kseg; kc0 += KC) {
            const int kc = min(KC, d.kseg - kc0);
            const int kcp = (kc + 3) & ~3;
            __syncthreads();
            for (int idx = tid; idx < ROWS * (kcp / 2); idx += 256) {
                const int rr = idx / (kcp / 2), c2 = idx % (kcp / 2);
                const int grow = row0 + rr;
                double v0 = 0.0, v1 = 0.0;
                if (grow < d.rows) {
                    const double* ap = d.A + (long long)(grow / d.rows_per_group) * d.a_group + (long long)(grow % d.rows_per_group) * d.a_row +
                                       (long long)seg * d.a_seg + kc0;
                    if (2 * c2 < kc) v0 = ap[2 * c2];
                    if (2 * c2 + 1 < kc) v1 = ap[2 * c2 + 1];
                }
                sm[rr * LD + 2 * c2] = v0;
                sm[rr * LD + 2 * c2 + 1] = v1;
            }
            __syncthreads();
            if (!wave_live) continue;
            const double* bp = d.B + ((long long)seg * d.kseg + kc0 + g) * d.ldb + col0 + r;
            const int krows = d.nseg * d.kseg;
            for (int t = 0; t < kcp / 4; ++t) {
                const int kglob = seg * d.kseg + kc0 + 4 * t + g;
                double bfr[NT], a[MT];
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int col = col0 + 16 * j + r;
                    bfr[j] = (col < d.ncols && 4 * t + g < kc && kglob < krows) ? bp[(long long)4 * t * d.ldb + 16 * j] : 0.0;
                }
#pragma unroll
                for (int i = 0; i < MT; ++i) a[i] = sm[(r + 16 * i) * LD + 4 * t + g];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    if (!wave_live) return;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int grow = row0 + 16 * i + g + 4 * q, col = col0 + 16 * j + r;
                if (grow < d.rows && col < d.ncols)
                    d.C[(long long)(grow / d.rows_per_group) * d.c_group + (long long)(grow % d.rows_per_group) * d.c_row +
                        (long long)(col / d.cols_per_group) * d.c_colgroup + (col % d.cols_per_group)] = acc[i][j][q];
            }
}

// Narrow outputs (templates projected onto a few dozen data bins; blockIdx.y walks column groups of 128 for wider ones): gemm_rows_kernel would run on a handful of
// workgroups, each walking the whole K serially.  Here a workgroup owns 16 rows, its four waves take a quarter of K each (all
// column tiles), and the quarters are added through LDS in a fixed order -- 4x the workgroups, 1/4 of the serial depth,
// bit-reproducible.  Same descriptor and addressing as gemm_rows_kernel.
constexpr int GN_MAXT = 8;  // column tiles of 16
constexpr int GN_MAXZ = 8;  // problems per launch (blockIdx.z): the per-tracer operators of one PROJECT stage
struct GemmZ {              // problem z reads A + z a_off, writes C + z c_off and multiplies by B[z] (all null / zero: one problem, d.B)
    const double* B[GN_MAXZ];
    long long a_off, c_off;
};
__global__ __launch_bounds__(256) void gemm_narrow_kernel(GemmDesc d, GemmZ z) {
    if (z.B[blockIdx.z]) {
        d.B = z.B[blockIdx.z];
        d.A += blockIdx.z * z.a_off;
        d.C += blockIdx.z * z.c_off;
    }
    __shared__ double red[3 * GN_MAXT * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * 16, c0 = blockIdx.y * 16 * GN_MAXT, nt = min(GN_MAXT, (d.ncols - c0 + 15) / 16);
    const int K = d.nseg * d.kseg, kq = ((K + 15) / 16) * 4;  // K quarter, a multiple of 4
    const int k0 = wave * kq, k1 = min(K, k0 + kq);
    const int grow = row0 + r;
    const bool rlive = grow < d.rows;
    const double* arow = d.A + (long long)((rlive ? grow : 0) / d.rows_per_group) * d.a_group + (long long)((rlive ? grow : 0) % d.rows_per_group) * d.a_row;
    v4d acc[GN_MAXT];
#pragma unroll
    for (int j = 0; j < GN_MAXT; ++j) acc[j] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int kb = k0; kb < k1; kb += 16) {  // four k-steps per trip: their loads are in flight together
        double a[4], bv[4][GN_MAXT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kk = kb + 4 * u + g;
            const bool klive = kk < k1;
            const int seg = klive ? kk / d.kseg : 0, kin = klive ? kk % d.kseg : 0;
            a[u] = (rlive && klive) ? arow[(long long)seg * d.a_seg + kin] : 0.0;
            const double* bp = d.B + (long long)(klive ? kk : 0) * d.ldb + c0 + r;
#pragma unroll
            for (int j = 0; j < GN_MAXT; ++j) bv[u][j] = (j < nt && klive && c0 + 16 * j + r < d.ncols) ? bp[16 * j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < GN_MAXT; ++j)
                if (j < nt) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bv[u][j], acc[j], 0, 0, 0);  // nt: workgroup-uniform
    }
    if (wave > 0)
#pragma unroll
        for (int j = 0; j < GN_MAXT; ++j)
            if (j < nt)
#pragma unroll
                for (int q = 0; q < 4; ++q) red[(((wave - 1) * GN_MAXT + j) * 4 + q) * 64 + lane] = acc[j][q];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int j = 0; j < GN_MAXT; ++j)
        if (j < nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double v = ((acc[j][q] + red[((0 * GN_MAXT + j) * 4 + q) * 64 + lane]) + red[((1 * GN_MAXT + j) * 4 + q) * 64 + lane]) +
                                 red[((2 * GN_MAXT + j) * 4 + q) * 64 + lane];
                const int orow = row0 + g + 4 * q, col = c0 + 16 * j + r;
                if (orow < d.rows && col < d.ncols)
                    d.C[(long long)(orow / d.rows_per_group) * d.c_group + (long long)(orow % d.rows_per_group) * d.c_row +
                        (long long)(col / d.cols_per_group) * d.c_colgroup + (col % d.cols_per_group)] = v;
            }
}

// ------------------------------------------------------------------------------------------------
// regroup: Bird.setPsCfl -- multipole weights, 28+10 -> 12 bias groups with powers of f, shot-noise
// subtraction, stochastic templates (reference pybird.py:737-866).  grp[b] = (group, power of f).
// Writes the template block T[w][l][24][Nk].
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void regroup_kernel(int Nk, int Nl, const double* __restrict__ kk, const double* __restrict__ fgrow,
                                                      const double* __restrict__ P11, const double* __restrict__ P22,
                                                      const double* __restrict__ P13, const double* __restrict__ l11,
                                                      const double* __restrict__ lct, const double* __restrict__ l22,
                                                      const double* __restrict__ l13, const int* __restrict__ grp,
                                                      double* __restrict__ T) {
    // one lane = one k of one (cosmology, multipole): reads the 28 + 10 loop pieces and writes the 24 template rows of its l.  The pieces are
    // walked group by group (each piece belongs to exactly one of the 12 bias groups; the lists are built per workgroup from the index map),
    // loaded when they are needed: no 38-entry register array, no select per (piece, group) pair
    __shared__ double cf[38];  // f^power * mu-weight per piece
    __shared__ double p0[38];  // the pieces at the first k (shot-noise subtraction, reference pybird.py:799-800)
    __shared__ int lst[12][38];
    __shared__ int cnt[12];
    const int k = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y, l = blockIdx.z;
    const double f = fgrow[w];
    for (int b = threadIdx.x; b < 38; b += blockDim.x) {
        cf[b] = ipow(f, grp[2 * b + 1]) * (b < 28 ? l22[l * 28 + b] : l13[l * 10 + (b - 28)]);
        p0[b] = b < 28 ? P22[((size_t)w * 28 + b) * Nk] : P13[((size_t)w * 10 + (b - 28)) * Nk];
    }
    if (threadIdx.x < 12) {  // pieces of group threadIdx.x, in ascending order (the order the sums have always been taken in)
        int n = 0;
        for (int b = 0; b < 38; ++b)
            if (grp[2 * b] == (int)threadIdx.x) lst[threadIdx.x][n++] = b;
        cnt[threadIdx.x] = n;
    }
    __syncthreads();
    if (k >= Nk) return;
    const double kv = kk[k], p11 = P11[(size_t)w * Nk + k];
    const double* q22 = P22 + (size_t)w * 28 * Nk + k;
    const double* q13 = P13 + (size_t)w * 10 * Nk + k;
    double* t = T + ((size_t)w * Nl + l) * NROW * Nk + k;
#pragma unroll
    for (int r = 0; r < 3; ++r) t[(size_t)r * Nk] = l11[l * 3 + r] * p11;
#pragma unroll
    for (int r = 0; r < 6; ++r) t[(size_t)(3 + r) * Nk] = lct[l * 6 + r] * kv * kv * p11;
    for (int i = 0; i < 12; ++i) {
        const int n = cnt[i];  // workgroup-uniform
        double acc = 0.0;
        for (int j = 0; j < n; ++j) {
            const int b = lst[i][j];
            const double d = (b < 28 ? q22[(size_t)b * Nk] : q13[(size_t)(b - 28) * Nk]) - p0[b];
            acc += cf[b] * d;
        }
        t[(size_t)(9 + i) * Nk] = acc;
    }
    t[(size_t)21 * Nk] = l == 0 ? 1.0 : 0.0;
    t[(size_t)22 * Nk] = l == 0 ? kv * kv : 0.0;
    t[(size_t)23 * Nk] = l == 1 ? kv * kv : 0.0;
}


// rows 21, 22, 23 of a template block (the stochastic templates Pstl; reference pybird.py:779-786): 1, k^2 at l = 0, k^2 at l = 2 -- functions of (l, k) alone
__device__ __forceinline__ double stoch_template(int l, int r, double kv) {
    return r == 0 ? (l == 0 ? 1.0 : 0.0) : r == 1 ? (l == 0 ? kv * kv : 0.0) : (l == 1 ? kv * kv : 0.0);
}

// Direct-P_l runs (EFTB_O_PLK_DIRECT): the bias contraction P_l = sum_row b_row T[l][row] commutes with every stage behind the regrouping
// (resummation, AP: linear maps that act on each template row alike), so it is taken FIRST: one row per multipole instead of 24 goes through
// them -- and, being linear in the rows, with the synthesis of the loop pieces before it (build_rows_plk_kernel).  This kernel is what is left of
// regroup_kernel (reference pybird.py:737-866 followed by parambasis.py:42-136): row 0 of the template block takes sum_row b_row T[l][row] over the
// rows the AP stage distorts (rows < 21, all rows when stoch0); rows 1-23 of the block are not written (the AP kernels of direct runs add the
// stochastic templates, stoch_template(), with their coefficients: round 4 -- they used to be stored here and read back there, 19 MB each way per 512 cosmologies).
__device__ __forceinline__ void regroup_plk_body(int kx, int w, int Nk, int Nl, const double* __restrict__ kk, const double* __restrict__ P11,
                                                 const double* __restrict__ Y22, const double* __restrict__ P13,
                                                 const double* __restrict__ l11, const double* __restrict__ lct,
                                                 const double* __restrict__ bias, double* __restrict__ T, int stoch0) {
    // Y22[w][l][k] (row stride BAS22 Nk per cosmology), P13[w][l][k] (10 Nk per cosmology): the loop pieces already contracted with the
    // bias (build_rows_plk_kernel) and synthesised; here the linear and counter terms join, the values at the first k are subtracted
    // (shot-noise subtraction, reference pybird.py:799-800) and the stochastic templates are laid beside the row.  A thread takes its k for
    // every l (round 4: a third of the waves of the per-(k, l) form, the same arithmetic per output)
    const int k = kx * 256 + threadIdx.x;   // (one workgroup = 256 k: the launch may carry more threads than that)
    if (threadIdx.x >= 256 || k >= Nk) return;
    const double* bw = bias + (size_t)w * NROW;
    const double kv = kk[k], p11 = P11[(size_t)w * Nk + k];
    double y22[3], q13[3], y0[3], q0[3];
#pragma unroll
    for (int l = 0; l < 3; ++l)
        if (l < Nl) {
            const double* yr = Y22 + ((size_t)w * BAS22 + l) * Nk;
            const double* qr = P13 + ((size_t)w * 10 + l) * Nk;
            y22[l] = yr[k]; y0[l] = yr[0]; q13[l] = qr[k]; q0[l] = qr[0];
        }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l >= Nl) break;
        double b11 = 0.0, bct = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) b11 = fma(bw[r], l11[l * 3 + r], b11);
#pragma unroll
        for (int r = 0; r < 6; ++r) bct = fma(bw[3 + r], lct[l * 6 + r], bct);
        const double s21 = l == 0 ? 1.0 : 0.0, s22 = l == 0 ? kv * kv : 0.0, s23 = l == 1 ? kv * kv : 0.0;
        double tot = (b11 + bct * kv * kv) * p11 + ((y22[l] - y0[l]) + (q13[l] - q0[l]));
        if (stoch0) tot += bw[21] * s21 + bw[22] * s22 + bw[23] * s23;  // APst: the stochastic templates are distorted with the others
        T[((size_t)w * Nl + l) * NROW * Nk + k] = tot;
    }
}

// optiresum: the BAO peak of every xi piece (one workgroup = one series of 80 s slots; reference pybird.py:1382-1400)
__global__ __launch_bounds__(128) void extract_bao_kernel(const double* __restrict__ bao, const double* __restrict__ in, double* __restrict__ out) {
    const int s = threadIdx.x;
    if (s >= NS) return;
    const int ilo = (int)bao[2 * NS], ihi = (int)bao[2 * NS + 1], i0 = (int)bao[2 * NS + 2], i1 = (int)bao[2 * NS + 3];
    const double* c = in + (size_t)blockIdx.x * NS;
    out[(size_t)blockIdx.x * NS + s] = (s >= i0 && s < i1) ? c[s] - bao[s] * c[ilo] - bao[NS + s] * c[ihi] : 0.0;
}

// NNLO block: rows 3-5 = k^4 P11 lctNNLO (reference pybird.py:741-748), every other row zero.  lctn is [Nl][6] (zero padded).
__global__ __launch_bounds__(256) void nnlo_rows_kernel(int Nk, int Nl, const double* __restrict__ kk, const double* __restrict__ P11,
                                                        const double* __restrict__ lctn, double* __restrict__ T) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y, l = blockIdx.z;
    if (k >= Nk) return;
    const double kv = kk[k], k4p = kv * kv * kv * kv * P11[(size_t)w * Nk + k];
    double* t = T + ((size_t)w * Nl + l) * NROW * Nk + k;
#pragma unroll
    for (int r = 0; r < NROW; ++r) t[(size_t)r * Nk] = (r >= 3 && r < 6) ? lctn[l * 6 + (r - 3)] * k4p : 0.0;
}

// Cloopl[w][l][12][80] from CC[w][Nl*38][80] (C22 then C13; reference pybird.py:752-753, 805-846)
__global__ __launch_bounds__(128) void regroup_cf_kernel(int Nl, const double* __restrict__ fgrow, const double* __restrict__ CC,
                                                         const double* __restrict__ l22, const double* __restrict__ l13,
                                                         const int* __restrict__ grp, double* __restrict__ Cloopl) {
    const int s = threadIdx.x, i = blockIdx.x, l = blockIdx.y, w = blockIdx.z;
    if (s >= NS) return;
    const double f = fgrow[w];
    const double* cc = CC + (size_t)w * Nl * 38 * NS;
    double a = 0.0;
    for (int b = 0; b < 28; ++b)
        if (grp[2 * b] == i) a += ipow(f, grp[2 * b + 1]) * l22[l * 28 + b] * cc[(size_t)(l * 28 + b) * NS + s];
    for (int b = 0; b < 10; ++b)
        if (grp[2 * (28 + b)] == i)
            a += ipow(f, grp[2 * (28 + b) + 1]) * l13[l * 10 + b] * cc[(size_t)(Nl * 28 + l * 10 + b) * NS + s];
    Cloopl[(((size_t)w * Nl + l) * 12 + i) * NS + s] = a;
}

// ------------------------------------------------------------------------------------------------
// Q(f) by Horner (reference pybird.py:1367-1380; the IR filters X(s), Y(s) come out of the first-stage GEMMs, see prep_rows_kernel).
// One workgroup per cosmology; Q[a] = table[1 - a] (pybird.py:1374-1376), nq = Nl*Nl*Nn entries per table.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qf_kernel(int nq, const double* __restrict__ fgrow, const double* __restrict__ Qpoly, double* __restrict__ Q) {
    qf_body(blockIdx.x, nq, fgrow, Qpoly, Q);
}

// ------------------------------------------------------------------------------------------------
// resum: the whole of Resum.Ps after the filters (reference pybird.py:1409-1462) collapsed to
//   W_a[l,l'](k,s) = sum_v H[v](k,s) * sum_j Q_a[l,l',j*Na+v] * phi_j(k,s),
//   phi_j = (k^2 X)^(j+1) (j < NIR),  k^2 Y (k^2 X)^(j-NIR) (j >= NIR)
//   P11l += sum_{l',s} l11[l',i] W_0 C11[l',s];  Pctl += ... lct W_1 Cct;  Ploopl += W_1 Cloopl[l',i,s]
// H folds the 192-point FFTLog of XpYp*C and the j_{2v} Bessel sum (tables.py).  Lanes along k, the s
// range is split over blockIdx.y (partials summed by resum_sum_kernel when nchunk > 1).
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// IR-resummation on the FP64 matrix cores (Nl = 3; tables.py resum_mfma_tables).
// All 108 polynomials  sum_p Q_a[l,l',(half,p,v)](f) z^p  of one cosmology lie in a fixed 8-dimensional space, so with
// an orthonormal basis beta_r(t), t = z / RS_ZS, of that space their values at 16 (k, s) points are one
// [rows x 8] x [8 x 16] product.  The weight of an (a, l, l') block is
//     W_a[l,l'](k,s) = k^2 sum_v H_v(k,s) [ delta(v,l') X(s) D(half 0, v) + Y(s) D(half 1, v) ],
// linear in the rows of the A operand, so the operand is built PER s (resum_as_kernel, [w][s][4 tiles][64 lanes][2]: the two
// doubles a lane feeds the two MFMAs of a tile; a function of the inputs alone, built beside the look-ahead chain) with X(s), Y(s)
// folded into its rows: three rows (v = 0, 1, 2) per block instead of four -- 18 blocks = 54 rows in four row tiles.  The four
// numbers a lane receives from one v_mfma_f64_16x16x4 (rows (lane >> 4) + 4 q, column lane & 15) are, for lane (jg = lane >> 4,
// n = lane & 15) at k = k0 + n:
//     tiles 0-2 (l' = tau), jg < 3:  q = 0..2 -> (a = 1, l = jg), v = q;     q = 3 -> (a = 0, l = 1, l' = tau), v = jg
//     tiles 0-2,            jg = 3:  q = 0..2 -> (a = 0, l = 0, l' = tau);   q = 3 -> zero row
//     tile 3,               jg < 3:  q = 0..2 -> (a = 0, l = 2, l' = jg);    everything else zero
// so every lane forms  W = H_0 D0 + H_1 D1 + H_2 D2  per tile and contracts it with the s-dependent (wave-uniform, scalar-loaded)
// C11 / Cct / Cloopl columns into its own output rows, accumulated over s in registers (fourth slot: H_jg C11[l'] D3, summed over the
// three lane groups after the loop; tile 3: the lane group's own C11 column, one vector load).  k^2 and the mu weights l11 / lct
// multiply the s-sums once, at the end.  The loop has no branches and no lane-role selects (hipcc shuffles MFMA results through AGPRs
// otherwise).  Per step: 8 MFMAs + 95 FP64 vector instructions (ten + 106, and 12 selects, with one four-slot operand per cosmology).
// resum_prep_kernel builds the per-s records
//   RSC[w][s] = { [l'][14]: C11[l'], Cct[l'], Cloopl[l',0..11] } , X, Y, pad  (48 doubles).
// (Nl = 2, resum_mfma2_kernel: one operand per cosmology, A = Q(f) diag(RS_ZS^p) V8^T, four-slot blocks.)
// ------------------------------------------------------------------------------------------------
constexpr double RS_ZS = 8.0;  // tables.py RS_ZS
constexpr int RS_NB = 8, RS_ROWS = 80, RS_REC = 48;
constexpr int RS3_TILES = 4, RS3_ROWS = 16 * RS3_TILES, RS3_AS = RS3_ROWS * RS_NB;  // Nl = 3: rows / doubles of one per-s operand
constexpr int RS_PF = 3;  // steps the Nl = 3 kernel prefetches its operand and records ahead (both buffers carry RS_PF spare steps)

template <int NL>
__global__ __launch_bounds__(256) void resum_prep_kernel(int NN, int NIR, int Na, const double* __restrict__ Q,
                                                         const double* __restrict__ V8S, const int* __restrict__ rows,
                                                         const double* __restrict__ XY, const double* __restrict__ C11,
                                                         const double* __restrict__ Cct, const double* __restrict__ Cloopl,
                                                         double* __restrict__ RSA, double* __restrict__ RSC, const double* __restrict__ CctN,
                                                         const double* __restrict__ CC, const double* __restrict__ fgrow,
                                                         const double* __restrict__ l22, const double* __restrict__ l13,
                                                         const int* __restrict__ grp) {
    // CctN (with_nnlo, may be null): Bird.CctNNLO rides in the spare slots 44-46 of the record, for the NNLO accumulator of resum_mfma_kernel
    // CC (may be null): the regrouping of C22 / C13 into Cloopl (Bird.setPsCfl for the xi pieces, reference pybird.py:805-846) is done
    // here, straight into the records -- whole-pipeline runs then skip regroup_cf_kernel and the Cloopl buffer
    const int w = blockIdx.x;
    const double* q = Q + (size_t)w * 2 * NL * NL * NN;
    __shared__ double s_cf[NL * 38];  // f^power * mu-weight per piece and multipole
    __shared__ int s_lst[12][38], s_cnt[12];  // the pieces of each bias group, ascending (22 pieces first: the order of regroup_cf_kernel)
    if (CC) {
        const double f = fgrow[w];
        for (int e = threadIdx.x; e < NL * 38; e += blockDim.x) {
            const int lp = e / 38, bq = e % 38;
            s_cf[e] = ipow(f, grp[2 * bq + 1]) * (bq < 28 ? l22[lp * 28 + bq] : l13[lp * 10 + (bq - 28)]);
        }
        if (threadIdx.x < 12) {
            int n = 0;
            for (int b = 0; b < 38; ++b)
                if (grp[2 * b] == (int)threadIdx.x) s_lst[threadIdx.x][n++] = b;
            s_cnt[threadIdx.x] = n;
        }
        __syncthreads();
    }
    // blockIdx.y splits the work of one cosmology (gridDim.y = 1: all of it): part 0 also builds the A operand (Nl = 2; Nl = 3: resum_as_kernel)
    const int part = blockIdx.y, nparts = gridDim.y;
    for (int idx = threadIdx.x; idx < (part == 0 && NL != 3 ? RS_ROWS * RS_NB : 0); idx += blockDim.x) {
        const int row = idx / RS_NB, r = idx % RS_NB, off = rows[row];
        double a0 = 0.0, a1 = 0.0;
        if (off >= 0)
            for (int p = 0; p < NIR; p += 2) {
                a0 = fma(q[off + p * Na], V8S[r * 16 + p], a0);
                a1 = fma(q[off + (p + 1) * Na], V8S[r * 16 + p + 1], a1);
            }
        RSA[((size_t)w * RS_ROWS + row) * RS_NB + r] = a0 + a1;
    }
    for (int idx = part * blockDim.x + threadIdx.x; idx < NS * RS_REC; idx += nparts * blockDim.x) {
        const int c = idx / NS, s = idx % NS;  // s fastest: coalesced reads of the s-major inputs
        double v = 0.0;
        if (c < 14 * NL) {
            const int lp = c / 14, j = c % 14;
            if (j == 0) v = C11[((size_t)w * NL + lp) * NS + s];
            else if (j == 1) v = Cct[((size_t)w * NL + lp) * NS + s];
            else if (!CC) v = Cloopl[(((size_t)w * NL + lp) * 12 + (j - 2)) * NS + s];
            else {  // same sums, in the same order, as regroup_cf_kernel
                const double* cc = CC + (size_t)w * NL * 38 * NS;
                const int n = s_cnt[j - 2];
                for (int t = 0; t < n; ++t) {
                    const int b = s_lst[j - 2][t];
                    v += s_cf[lp * 38 + b] * cc[(size_t)(b < 28 ? lp * 28 + b : NL * 28 + lp * 10 + (b - 28)) * NS + s];
                }
            }
        } else if (c < 44) {
            v = XY[(size_t)w * 2 * NS + (c - 42) * NS + s];
        } else if (CctN && c < 44 + NL) {
            v = CctN[((size_t)w * NL + (c - 44)) * NS + s];
        }
        RSC[((size_t)w * NS + s) * RS_REC + c] = v;
    }
}

// Per-s A operand of resum_mfma_kernel (Nl = 3; inputs only: Q(f), X(s), Y(s) -- off the look-ahead chain, memory-bound):
//   RSAS[w][s][tau][lane][t] = (X(s) a_X + Y(s) a_Y)[row 16 tau + (lane & 15)][column (lane >> 4) + 4 t],   a_X | a_Y = Q rows . V8S^T,
// rows[0 | 1][row] = offset of the row's X | Y part in the cosmology's Q block (-1: none).  Grid (cosmology, s quarter); a thread keeps its two
// entries of a_X, a_Y in registers and walks s: every store instruction of the workgroup writes 2 KB of consecutive addresses.
__global__ __launch_bounds__(256) void resum_as_kernel(int NN, int NIR, int Na, const double* __restrict__ Q, const double* __restrict__ V8S,
                                                       const int* __restrict__ rows, const double* __restrict__ XY, double* __restrict__ RSAS) {
    const int w = blockIdx.x;
    const double* q = Q + (size_t)w * 2 * 3 * 3 * NN;
    double ax[2], ay[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int e = threadIdx.x + 256 * j, tau = e >> 7, lane = (e >> 1) & 63, t = e & 1;
        const int row = 16 * tau + (lane & 15), r = (lane >> 4) + 4 * t;
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const int off = rows[which * RS3_ROWS + row];
            double a0 = 0.0, a1 = 0.0;
            if (off >= 0)
                for (int p = 0; p < NIR; p += 2) {
                    a0 = fma(q[off + p * Na], V8S[r * 16 + p], a0);
                    a1 = fma(q[off + (p + 1) * Na], V8S[r * 16 + p + 1], a1);
                }
            (which ? ay : ax)[j] = a0 + a1;
        }
    }
    const int ns = (NS + gridDim.y - 1) / gridDim.y, s0 = blockIdx.y * ns, s1 = min(NS, s0 + ns);
    const double* xy = XY + (size_t)w * 2 * NS;
    double* dst = RSAS + ((size_t)w * NS + s0) * RS3_AS + threadIdx.x;
    for (int s = s0; s < s1; ++s, dst += RS3_AS) {
        const double x = xy[s], y = xy[NS + s];
        dst[0] = fma(x, ax[0], y * ay[0]);
        dst[256] = fma(x, ax[1], y * ay[1]);
    }
}

__device__ inline double estrin16(const double* __restrict__ c, double t, double t2, double t4, double t8) {
    const double e0 = fma(c[1], t, c[0]), e1 = fma(c[3], t, c[2]), e2 = fma(c[5], t, c[4]), e3 = fma(c[7], t, c[6]);
    const double e4 = fma(c[9], t, c[8]), e5 = fma(c[11], t, c[10]), e6 = fma(c[13], t, c[12]), e7 = fma(c[15], t, c[14]);
    const double f0 = fma(e1, t2, e0), f1 = fma(e3, t2, e2), f2 = fma(e5, t2, e4), f3 = fma(e7, t2, e6);
    const double g0 = fma(f1, t4, f0), g1 = fma(f3, t4, f2);
    return fma(g1, t8, g0);
}

// NNLO: the k^4 P11 counter-terms PctNNLOl (reference pybird.py:1447-1458) take the same W as Pctl with CctNNLO in place of Cct and lctNNLO in
// place of lct -- three more accumulators per lane (record slots 44-46) instead of a second pass over the whole stage; TN is the NNLO
// block (rows 3-5).  Only with nsplit = 1 (the partial-sum layout of small batches has no slot for it: those run the second pass).
template <bool NNLO>
__global__ __launch_bounds__(256, 2) void resum_mfma_kernel(int Nk, int Nklow, int schunk, const double* __restrict__ kk,
                                                            const double* __restrict__ H, const double* __restrict__ V8,
                                                            const double* __restrict__ RSAS, const double* __restrict__ RSC,
                                                            const double* __restrict__ l11, const double* __restrict__ lct,
                                                            double* __restrict__ T, double* __restrict__ part, int nsplit,
                                                            const double* __restrict__ lctn, double* __restrict__ TN, int nkb) {
    constexpr int NL = 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int jg = lane >> 4, n = lane & 15;
    // Workgroup -> (k block, cosmology).  The k tiles start at a multiple of 16 (the 128-byte template segments of a wave are then whole
    // cache lines; lanes below Nklow idle), and the nkb workgroups of one cosmology sit on ONE XCD (consecutive workgroup ids go round the
    // eight XCDs): its per-s operands and records then pass through one L2 instead of eight.
    int kb, w;
    xcd_decode(nkb, kb, w);
    const int k = (Nklow & ~15) + (kb * 4 + wave) * 16 + n, split = blockIdx.z;
    const int kc = k < Nklow ? Nklow : (k < Nk ? k : Nk - 1);  // lanes outside [Nklow, Nk) compute on a clamped k and store nothing
    const double k2 = kk[kc] * kk[kc], k2t = k2 * (1.0 / RS_ZS);
    // B operand: this lane evaluates basis polynomials jg and jg + 4 at its point; A operand: rows (16 tau + n), columns jg + 4 t
    double vb[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < 16; ++p) vb[t][p] = V8[(jg + 4 * t) * 16 + p];
#define RS_POLY(out0, out1, tt)                                                        \
    do {                                                                               \
        const double t_ = (tt), t2_ = t_ * t_, t4_ = t2_ * t2_, t8_ = t4_ * t4_;       \
        out0 = estrin16(vb[0], t_, t2_, t4_, t8_);                                     \
        out1 = estrin16(vb[1], t_, t2_, t4_, t8_);                                     \
    } while (0)
    // s-sums: W Cloopl[l',i] (summed over l'), W Cct[l'] (jg < 3); W C11[l'] of the (a = 0, l = 0, l') block (jg = 3); H_jg D3 C11[l'] = the
    // v = jg part of the (a = 0, l = 1, l') block; tile 3: W C11[jg] of the (a = 0, l = 2, l' = jg) block
    double accL[12], accCt[3], accP[3], accQ[3], accP3 = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) accL[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) accCt[i] = accP[i] = accQ[i] = 0.0;
    double accN[3] = {0.0, 0.0, 0.0};  // NNLO: W CctNNLO[l']
    const int s0 = split * schunk, s1 = min(NS, s0 + schunk);
    const double* ct = RSC + ((size_t)w * NS + s0) * RS_REC;  // wave-uniform record of the current s
    // per-s A operand: one wave-uniform base and a 32-bit per-lane byte offset ([tau][lane][2]: a wave's load of a tile is 1 KB, contiguous)
    const char* as = reinterpret_cast<const char*>(RSAS + (size_t)w * NS * RS3_AS);
    unsigned aoff = (unsigned)s0 * (RS3_AS * 8u) + (unsigned)lane * 16u;
    // H[v][s][k]: one wave-uniform base and 32-bit per-lane byte offsets (64-bit per-lane pointers would cost the registers that
    // decide whether other kernels fit beside two of these waves on a SIMD); hq = H of the fourth slot's v = jg
    const char* Hb = reinterpret_cast<const char*>(H);
    const unsigned hrow = (unsigned)NS * (unsigned)Nk * 8u, hstep = (unsigned)Nk * 8u;
    unsigned hoff = ((unsigned)s0 * (unsigned)Nk + (unsigned)kc) * 8u;
    const unsigned hqv = (unsigned)(jg < 3 ? jg : 0) * hrow;
    // L2 prefetch RS_PF steps ahead: the operand of a step is first touched by the 32 waves of its cosmology together, an HBM / fabric round
    // trip that the one step between its request and its use does not cover.  One dword per lane, 64 B apart = the whole 4 KB operand
    // (lanes 0-5 of the second load: the 384 B record); the values are never used.
    // (no clamp at the end of the s range: both buffers are allocated RS_PF steps longer)
    unsigned pfoff = (unsigned)(s0 + RS_PF) * (RS3_AS * 8u) + (unsigned)lane * 64u;
    const char* rcb = reinterpret_cast<const char*>(RSC + (size_t)w * NS * RS_REC);
    unsigned pfroff = (unsigned)(s0 + RS_PF) * (RS_REC * 8u) + (unsigned)(lane < 6 ? lane : 0) * 64u;
    unsigned c11off = (unsigned)s0 * (RS_REC * 8u) + (unsigned)(jg < 3 ? jg : 0) * (14u * 8u);
    double h[3], hq, b0, b1;
    v2d aop[RS3_TILES];
#pragma unroll
    for (int v = 0; v < 3; ++v) h[v] = *reinterpret_cast<const double*>(Hb + (hoff + v * hrow));
    hq = *reinterpret_cast<const double*>(Hb + (hoff + hqv));
#pragma unroll
    for (int tau = 0; tau < RS3_TILES; ++tau) aop[tau] = *reinterpret_cast<const v2d*>((as + tau * 1024) + aoff);
    RS_POLY(b0, b1, k2t * ct[42]);
    for (int s = s0; s < s1; ++s) {
        // memory first: the prefetches, this step's C columns of l' = 0, 1 (scalar loads, consumed after the MFMAs; those of l' = 2 follow once
        // tile 0 has been consumed -- 42 doubles at once overflow the scalar file and come back as v_readlane traffic) and the next step's X
        const bool more = s + 1 < s1;
        const double* ctn = more ? ct + RS_REC : ct;
        const unsigned pf0 = *reinterpret_cast<const unsigned*>(as + pfoff), pf1 = *reinterpret_cast<const unsigned*>(rcb + pfroff);
        pfoff += RS3_AS * 8u;
        pfroff += RS_REC * 8u;
        aoff += more ? RS3_AS * 8u : 0u;
        asm volatile("" : "+v"(aoff));  // formed here, not behind the MFMAs (where it would land in a register they still read: 16 wait states)
        const double c11q = *reinterpret_cast<const double*>(rcb + c11off);  // C11[l' = jg](s) of this step: the column of the lane's tile-3 block
        c11off += more ? RS_REC * 8u : 0u;
        double cv[3][14];  // per l': C11, Cct, Cloopl[0..11]
#pragma unroll
        for (int tau = 0; tau < 2; ++tau)
#pragma unroll
            for (int i = 0; i < 14; ++i) cv[tau][i] = ct[tau * 14 + i];
        double cn[3] = {0.0, 0.0, 0.0};
        if (NNLO) {
#pragma unroll
            for (int i = 0; i < 3; ++i) cn[i] = ct[44 + i];
        }
        const double xn = ctn[42];
        __builtin_amdgcn_sched_barrier(0);
        // all eight MFMAs of this step (four independent accumulators) ...
        v4d D[RS3_TILES];
#pragma unroll
        for (int tau = 0; tau < RS3_TILES; ++tau) D[tau] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[tau][0], b0, (v4d){0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
#pragma unroll
        for (int tau = 0; tau < RS3_TILES; ++tau) D[tau] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[tau][1], b1, D[tau], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // ... the next step's operand is requested once they have been issued (same registers: the loads land while the vector work below runs)
#pragma unroll
        for (int tau = 0; tau < RS3_TILES; ++tau) aop[tau] = *reinterpret_cast<const v2d*>((as + tau * 1024) + aoff);
        __builtin_amdgcn_sched_barrier(0);
#define RS_USE(tau)                                                                                              \
    do {                                                                                                         \
        const double W_ = fma(h[0], D[tau][0], fma(h[1], D[tau][1], h[2] * D[tau][2]));                          \
        accP[tau] = fma(W_, cv[tau][0], accP[tau]);                                                              \
        accCt[tau] = fma(W_, cv[tau][1], accCt[tau]);                                                            \
        if (NNLO) accN[tau] = fma(W_, cn[tau], accN[tau]);                                                       \
        _Pragma("unroll") for (int i = 0; i < 12; ++i) accL[i] = fma(W_, cv[tau][2 + i], accL[i]);               \
        accQ[tau] = fma(hq * cv[tau][0], D[tau][3], accQ[tau]);                                                  \
    } while (0)
        // ... under them the contraction of this step and the basis polynomials of the next (k^2 X formed only now: the wait for the scalar
        // loads above then sits behind the matrix work instead of behind the first MFMA)
        RS_USE(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 14; ++i) cv[2][i] = ct[28 + i];
        double bn0, bn1;
        RS_POLY(bn0, bn1, k2t * xn);
        RS_USE(1);
        __builtin_amdgcn_sched_barrier(0);
        RS_USE(2);
        accP3 = fma(fma(h[0], D[3][0], fma(h[1], D[3][1], h[2] * D[3][2])), c11q, accP3);
#undef RS_USE
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::"v"(pf0), "v"(pf1));  // (the prefetches are older than the operand loads above)
        // the next step's H into the registers this step has just read for the last time (L2-resident table: back before the MFMAs are through)
        hoff += more ? hstep : 0u;
#pragma unroll
        for (int v = 0; v < 3; ++v) h[v] = *reinterpret_cast<const double*>(Hb + (hoff + v * hrow));
        hq = *reinterpret_cast<const double*>(Hb + (hoff + hqv));
        ct = ctn;
        b0 = bn0;
        b1 = bn1;
    }
#undef RS_POLY
    // (a, l) blocks -> output rows: k^2 and the mu weights applied to the s-sums.  The (a = 0, l = 1 | 2) sums are spread over the lane
    // groups jg < 3 (one v, or one l', each): gathered into the jg = 0 lane of every k.
    double o18[18], oA[3], o1[3], o2[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) o18[i] = k2 * (lct[i] * accCt[0] + lct[6 + i] * accCt[1] + lct[12 + i] * accCt[2]);
#pragma unroll
    for (int i = 0; i < 12; ++i) o18[6 + i] = k2 * accL[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        oA[i] = k2 * (l11[i] * accP[0] + l11[3 + i] * accP[1] + l11[6 + i] * accP[2]);
        const double t1 = jg < 3 ? l11[i] * accQ[0] + l11[3 + i] * accQ[1] + l11[6 + i] * accQ[2] : 0.0;
        const double t2 = jg < 3 ? l11[jg * 3 + i] * accP3 : 0.0;
        o1[i] = k2 * (t1 + __shfl(t1, (lane + 16) & 63) + __shfl(t1, (lane + 32) & 63));
        o2[i] = k2 * (t2 + __shfl(t2, (lane + 16) & 63) + __shfl(t2, (lane + 32) & 63));
    }
    if (k >= Nk || k < Nklow) return;
    if (nsplit == 1) {
        if (jg < 3) {
            double* dst = T + (((size_t)w * NL + jg) * NROW + 3) * Nk + k;
#pragma unroll
            for (int i = 0; i < 18; ++i) dst[(size_t)i * Nk] += o18[i];
            if (NNLO) {  // PctNNLOl[l = jg][i] += sum_l' lctNNLO[l'][i] W Cct_NNLO[l']   (lctn is [Nl][6], zero padded)
                double* dn = TN + (((size_t)w * NL + jg) * NROW + 3) * Nk + k;
#pragma unroll
                for (int i = 0; i < 3; ++i) dn[(size_t)i * Nk] += k2 * (lctn[i] * accN[0] + lctn[6 + i] * accN[1] + lctn[12 + i] * accN[2]);
            }
        } else {
            double* dst = T + (((size_t)w * NL + 0) * NROW) * Nk + k;
#pragma unroll
            for (int i = 0; i < 3; ++i) dst[(size_t)i * Nk] += oA[i];
        }
        if (jg == 0) {
            double* d1 = T + (((size_t)w * NL + 1) * NROW) * Nk + k;
            double* d2 = T + (((size_t)w * NL + 2) * NROW) * Nk + k;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                d1[(size_t)i * Nk] += o1[i];
                d2[(size_t)i * Nk] += o2[i];
            }
        }
    } else {  // partial sums over the s slices, added in a fixed order by resum_sum_kernel
        double* pw = part + ((size_t)w * nsplit + split) * NL * 21 * Nk + k;
        if (jg < 3) {
#pragma unroll
            for (int i = 0; i < 18; ++i) pw[((size_t)jg * 21 + 3 + i) * Nk] = o18[i];
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) pw[(size_t)i * Nk] = oA[i];
        }
        if (jg == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                pw[((size_t)21 + i) * Nk] = o1[i];
                pw[((size_t)42 + i) * Nk] = o2[i];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// IR-resummation of direct-P_l runs (EFTB_O_PLK_DIRECT; Nl = 3).  With the bias contraction taken first the correction of P_l is
//     dP_l(k) = k^2 sum_s sum_v H_v(k,s) D_lv(k^2 X(s); s),
//     D_lv(z; s) = sum_p z^p sum_l' sum_a g_a[l'](s) ( delta(v,l') X(s) Q_a[l,l',(0,p,v)] + Y(s) Q_a[l,l',(1,p,v)] ),
//     g_0[l'](s) = C11[l'](s) sum_i b_i l11[l'][i],    g_1[l'](s) = Cct[l'](s) sum_i b_3+i lct[l'][i] + sum_i b_9+i Cloopl[l'][i](s)
// (reference pybird.py:1413-1464 contracted with parambasis.py:42-136): nine polynomials of degree 15 per s whose coefficients are the same
// for every k.  All of them lie in one 8-dimensional space with a closed-form basis (tables.py resum_plk_tables): with u = -z / 2
//     sum_p q_p z^p = -1/2 sum_j c_j b_j(u),   b_0 = sum_{p<16} u^p / (p+1)!,   b_j = u^(j-1) e_{16-j}(u)  (j = 1..7),   e_n = sum_{m<=n} u^m / m!
// and the eight b_j fall out of ONE Horner evaluation of e_16: h_16 = 1/16!, h_m = h_{m+1} u + 1/m! gives h_m = sum_i u^i / (m+i)!, so
//     b_0 = h_1,   b_j = u^(j-1) h_0 - u^16 h_{17-j}.
// The basis costs 37 FP64 instructions per (k, s) and is shared by the nine (l, v): each is an 8-term dot product with SCALAR coefficients
// W[l][v][j](s) and one FMA with H_v -- 118 instructions per (k, s) where nine Horner chains of degree 15 took 162.  resum_prep_plk_kernel
// builds the records per cosmology (CF[w][s][80]: W [l][v][j] with the -1/2 folded in, then -X(s) / 2) from Q_e(f), the coordinates c_j of
// Q(f) (qf_body on the table QEpoly), with the regrouping of C22 / C13 into Cloopl (pybird.py:805-846) folded into g_1.
// ------------------------------------------------------------------------------------------------
constexpr int RSD_NB = 8;    // basis functions
constexpr int RSD_REC = 80;  // doubles per (cosmology, s): 9 x 8 coefficients, -X / 2, pad
constexpr int RSD_NN = 2 * RSD_NB * 3;  // Q_e(f) entries per (a, l, l'): [half][j][v]
constexpr int RSD_KPL = 2, RSD_SH = 8;  // the shape resum_plk_kernel is launched in: k per lane, slices of the s range

__device__ __forceinline__ void resum_prep_plk_body(int w, int part, int nparts, const double* __restrict__ Q,
                                                    const double* __restrict__ XY, const double* __restrict__ C11, const double* __restrict__ Cct,
                                                    const double* __restrict__ YCF, double* __restrict__ CF) {
    // grid (cosmology, slice of the s range).  g_0[l'](s) = C11[w][l'][s], g_1[l'](s) = Cct[w][l'][s] + YCF[w][l'][s]: all three already carry their
    // bias coefficients (build_rows_plk_kernel contracted the rows before the synthesis).  A thread owns ONE entry c = (l, v, j) of the record
    // and walks every fourth s of the slice: its eight Q_e(f) values sit in registers, g, X and Y of the slice in LDS (broadcast reads) -- the
    // first form (entries x s flattened over the workgroup, X / Y from global memory inside the loop, Q(f) in LDS) took ten dependent global
    // loads per thread: 29 us alone at 512 cosmologies per launch, a third of them in a second round of workgroups
    constexpr int NL = 3, Na = 3, NN = RSD_NN;
    const int ns = (NS + nparts - 1) / nparts, s0 = part * ns, s1 = min(NS, s0 + ns), nsl = s1 - s0;
    extern __shared__ double sm[];
    double* s_g = sm;                  // [2][NL][ns] g_a[l'](s0 + .)
    double* s_xy = sm + 2 * NL * ns;   // [2][ns] X, Y
    for (int e = threadIdx.x; e < NL * nsl; e += blockDim.x) {
        const int lp = e / nsl, sl = e % nsl, s = s0 + sl;
        s_g[lp * ns + sl] = C11[((size_t)w * NL + lp) * NS + s];
        s_g[(NL + lp) * ns + sl] = Cct[((size_t)w * NL + lp) * NS + s] + YCF[((size_t)w * BASC + lp) * NS + s];
    }
    for (int e = threadIdx.x; e < 2 * nsl; e += blockDim.x) s_xy[(e / nsl) * ns + e % nsl] = XY[(size_t)w * 2 * NS + (size_t)(e / nsl) * NS + s0 + e % nsl];
    const int c = threadIdx.x % RSD_REC, quarter = threadIdx.x / RSD_REC, nquarter = blockDim.x / RSD_REC;
    const int l = c / (3 * RSD_NB), vv = (c / RSD_NB) % 3, j = c % RSD_NB;
    const bool poly = c < 9 * RSD_NB;
    double qy[2][NL], qx[2] = {0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 2; ++a)   // device Q[a]: 0 = the C11 series, 1 = the Cct / Cloopl series
#pragma unroll
        for (int lp = 0; lp < NL; ++lp) {
            qy[a][lp] = 0.0;
            if (poly) {
                const double* qq = Q + (size_t)w * 2 * NL * NL * NN + ((a * NL + l) * NL + lp) * NN + j * Na + vv;
                qy[a][lp] = qq[RSD_NB * Na];
                if (lp == vv) qx[a] = qq[0];
            }
        }
    __syncthreads();
    double* dst = CF + ((size_t)w * NS + s0) * RSD_REC + c;
    for (int sl = quarter; sl < nsl; sl += nquarter) {
        double v = 0.0;
        if (poly) {
            const double x = s_xy[sl], y = s_xy[ns + sl];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int lp = 0; lp < NL; ++lp) {
                    double term = y * qy[a][lp];
                    if (lp == vv) term = fma(x, qx[a], term);
                    v = fma(s_g[(a * NL + lp) * ns + sl], term, v);
                }
            v *= -0.5;
        } else if (c == 9 * RSD_NB) {
            v = -0.5 * s_xy[sl];
        }
        dst[(size_t)sl * RSD_REC] = v;
    }
}

// One launch for the two light kernels between the syntheses and the resummation of a direct-P_l run (a launch costs the host 4 us and the step is
// bounded by the host): workgroups [0, nreg) = regroup_plk (k tile, cosmology, l), the rest = resum_prep_plk (cosmology, slice of the s range)
constexpr int BPP_THREADS = 4 * RSD_REC;   // 320: the coefficient part's (entry, quarter of the s slice); the regrouping part uses the first 256
__global__ __launch_bounds__(BPP_THREADS) void back_prep_plk_kernel(int nreg, int nkx, int B, int nparts, int Nk, int Nl, const double* __restrict__ kk,
                                                            const double* __restrict__ P11, const double* __restrict__ Y22,
                                                            const double* __restrict__ P13, const double* __restrict__ l11,
                                                            const double* __restrict__ lct, const double* __restrict__ bias, double* __restrict__ T,
                                                            int stoch0, const double* __restrict__ Q,
                                                            const double* __restrict__ XY, const double* __restrict__ C11,
                                                            const double* __restrict__ Cct, const double* __restrict__ YCF, double* __restrict__ CF) {
    const int id = blockIdx.x;
    if (id < nreg) {
        regroup_plk_body(id % nkx, id / nkx, Nk, Nl, kk, P11, Y22, P13, l11, lct, bias, T, stoch0);
    } else {
        const int j = id - nreg;
        resum_prep_plk_body(j % B, j / B, nparts, Q, XY, C11, Cct, YCF, CF);
    }
}

// FP64 vector operations with one scalar (wave-uniform) operand, spelled out
__device__ __forceinline__ double sop_fma(double a, double b, double c) {   // a b + c, c scalar
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}
__device__ __forceinline__ double sop_fmas(double a, double b, double c) {  // a b + c, b scalar
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}
__device__ __forceinline__ double sop_fnmas(double a, double b, double c) {  // c - a b, b scalar
    double r;
    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}
__device__ __forceinline__ double sop_mul(double a, double c) {
    double r;
    asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(c));
    return r;
}

// 1 / m!, m = 0 ... 16: the Horner coefficients of e_16.  A 64-bit constant cannot be a literal operand, so each one the loop uses is a scalar
// register pair (sop_fma) -- 1, 1, 1/2 are inline constants and 1/15! sits in a vector pair.  (The other way, the constants as per-s Horner
// coefficients in k^2 riding in the record, was not built: it adds 16 scalar loads per s to a kernel whose remaining waits are scalar loads.
// With the ring below the thirteen pairs no longer all fit beside it: the compiler keeps some in lanes of a vector register, 27 v_readlane /
// v_writelane per s step -- still the faster form, 29.3 us alone at 128 cosmologies against 31.1 with sets of eight and every constant resident.)
__host__ __device__ constexpr double rsd_inv_fact(int m) {
    double f = 1.0;
    for (int i = 2; i <= m; ++i) f *= i;
    return 1.0 / f;
}
#define RSD_F(m) rsd_inv_fact(m)

// workgroup = SH waves = slices of the s range of one (64 KPL k, cosmology): a lane owns KPL k (64 apart), and a wave owns ALL nine (l, v) of
// its (k, s) points -- the eight basis values of a point live in registers and serve nine dot products (shared between waves through LDS
// each value would be read back for a single FMA: a CU's LDS returns 16 doubles per clock against 64 FP64 lanes).  Per s a wave reads its 72
// scalar coefficients through a ring of two sets of sixteen (two dot products each) and one of eight: a set is requested at least two dot
// products (36 FP64 instructions per k) before it is read and waited for where it is first used (scalar loads return out of order: a wait
// is always for all of them, so it must not sit behind the requests of the next set) -- four waits per s; with sets of eight, ten waits
// per s and one dot product of cover, four resident waves did not hide the loads (31.1 us alone against 29.3).  The SH partial sums of the three l meet in LDS at the end and are added in wave order: no atomics, the result
// does not depend on timing.  KPL = 2, SH = 8: 4 096 equal waves per 128 cosmologies = four per SIMD.
template <int KPL, int SH>
__global__ __launch_bounds__(64 * SH, 4) void resum_plk_kernel(int Nk, int Nklow, const double* __restrict__ kk, const double* __restrict__ H,
                                                               const double* __restrict__ CF, double* __restrict__ T, int KT) {
    constexpr int NL = 3, NV = 3, NSH = NS / SH;
    static_assert(NS % (2 * SH) == 0, "two s steps per trip");
    __shared__ double s_part[SH - 1][NL][KPL][64];
    const int lane = threadIdx.x & 63, sh = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (wave-uniform: the coefficient loads stay scalar)
    // workgroup -> (k tile of 64 KPL, cosmology); the KT workgroups of a cosmology sit on one XCD (its coefficient table passes through one L2)
    int kt, w;
    xcd_decode(KT, kt, w);
    int k[KPL];
    double k2[KPL], acc[NL][KPL], h[NV][KPL];
    const double* hp = H + (size_t)sh * NSH * Nk;
    const size_t hv = (size_t)NS * Nk;
    unsigned ho[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        k[i] = kt * 64 * KPL + 64 * i + lane;
        const int kc = k[i] < Nklow ? Nklow : (k[i] < Nk ? k[i] : Nk - 1);  // lanes outside [Nklow, Nk) compute on a clamped k and store nothing
        k2[i] = kk[kc] * kk[kc];
        ho[i] = (unsigned)kc;
#pragma unroll
        for (int v = 0; v < NV; ++v) h[v][i] = hp[v * hv + ho[i]];
#pragma unroll
        for (int l = 0; l < NL; ++l) acc[l][i] = 0.0;
    }
    const double* cf = CF + ((size_t)w * NS + sh * NSH) * RSD_REC;  // wave-uniform: scalar loads; -X / 2 sits at [72] of the record
    const double f15 = RSD_F(15);
    // the ring: two sets of sixteen coefficients = two (l, v) each, and one of eight for the ninth
    double ca[2 * RSD_NB], cb[2 * RSD_NB], cc[RSD_NB], xa = cf[9 * RSD_NB];
#pragma unroll
    for (int j = 0; j < 2 * RSD_NB; ++j) ca[j] = cf[j];
    double b[KPL][RSD_NB], hn[NV][KPL];
    // the dot product of (l, v) = Q with the basis, times H_v, into the sum of l; its eight coefficients start at CUR[O]
#define RSD_MAC(CUR, O, Q)                                                                                  \
    do {                                                                                                    \
        double d[KPL];                                                                                      \
        _Pragma("unroll") for (int i = 0; i < KPL; ++i) d[i] = sop_mul(b[i][0], CUR[O]);                    \
        _Pragma("unroll") for (int j = 1; j < RSD_NB; ++j)                                                  \
            _Pragma("unroll") for (int i = 0; i < KPL; ++i) d[i] = sop_fmas(b[i][j], CUR[(O) + j], d[i]);   \
        _Pragma("unroll") for (int i = 0; i < KPL; ++i) acc[(Q) / NV][i] = fma(h[(Q) % NV][i], d[i], acc[(Q) / NV][i]); \
    } while (0)
#define RSD_WAIT(...)                                                                                       \
    asm volatile("" ::__VA_ARGS__); /* the wait for a set: in front of the next requests */                 \
    __builtin_amdgcn_sched_barrier(0)
    // one s.  On entry ca holds the sets (l, v) = 0, 1 and xa the scalar -X(s) / 2, requested during the previous step
#define RSD_STEP(MORE)                                                                                      \
    do {                                                                                                    \
        RSD_WAIT("s"(ca[0]), "s"(xa));                                                                      \
        const double* cfn = cf + ((MORE) ? RSD_REC : 0);                                                    \
        hp += (MORE) ? Nk : 0;                                                                              \
        _Pragma("unroll") for (int j = 0; j < 2 * RSD_NB; ++j) cb[j] = cf[2 * RSD_NB + j];                  \
        _Pragma("unroll") for (int i = 0; i < KPL; ++i)                                                     \
            _Pragma("unroll") for (int v = 0; v < NV; ++v) hn[v][i] = hp[v * hv + ho[i]];                   \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        _Pragma("unroll") for (int i = 0; i < KPL; ++i) {                                                   \
            const double u = sop_mul(k2[i], xa);                                                            \
            double g[17];                                                                                   \
            g[15] = sop_fmas(u, RSD_F(16), f15);                                                            \
            _Pragma("unroll") for (int m = 14; m >= 3; --m) g[m] = sop_fma(g[m + 1], u, RSD_F(m));          \
            g[2] = fma(g[3], u, 0.5);                                                                       \
            g[1] = fma(g[2], u, 1.0);                                                                       \
            g[0] = fma(g[1], u, 1.0);                                                                       \
            const double u2 = u * u, u3 = u2 * u, u4 = u2 * u2, u5 = u4 * u, u6 = u4 * u2, u8 = u4 * u4, u16 = u8 * u8; \
            const double pw[7] = {1.0, u, u2, u3, u4, u5, u6};                                              \
            b[i][0] = g[1];                                                                                 \
            b[i][1] = sop_fnmas(u16, RSD_F(16), g[0]);                                                      \
            _Pragma("unroll") for (int j = 2; j < RSD_NB; ++j) {                                            \
                const double t = u16 * g[17 - j];                                                           \
                b[i][j] = fma(pw[j - 1], g[0], -t);                                                         \
            }                                                                                               \
        }                                                                                                   \
        RSD_MAC(ca, 0, 0);                                                                                  \
        RSD_MAC(ca, RSD_NB, 1);                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        RSD_WAIT("s"(cb[0]));                                                                               \
        _Pragma("unroll") for (int j = 0; j < 2 * RSD_NB; ++j) ca[j] = cf[4 * RSD_NB + j];                  \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        RSD_MAC(cb, 0, 2);                                                                                  \
        RSD_MAC(cb, RSD_NB, 3);                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        RSD_WAIT("s"(ca[0]));                                                                               \
        _Pragma("unroll") for (int j = 0; j < 2 * RSD_NB; ++j) cb[j] = cf[6 * RSD_NB + j];                  \
        _Pragma("unroll") for (int j = 0; j < RSD_NB; ++j) cc[j] = cf[8 * RSD_NB + j];                      \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        RSD_MAC(ca, 0, 4);                                                                                  \
        RSD_MAC(ca, RSD_NB, 5);                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        RSD_WAIT("s"(cb[0]), "s"(cc[0]));                                                                   \
        _Pragma("unroll") for (int j = 0; j < 2 * RSD_NB; ++j) ca[j] = cfn[j];                              \
        xa = cfn[9 * RSD_NB];                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        RSD_MAC(cb, 0, 6);                                                                                  \
        RSD_MAC(cb, RSD_NB, 7);                                                                             \
        RSD_MAC(cc, 0, 8);                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        cf = cfn;                                                                                           \
        _Pragma("unroll") for (int i = 0; i < KPL; ++i)                                                     \
            _Pragma("unroll") for (int v = 0; v < NV; ++v) h[v][i] = hn[v][i];                              \
    } while (0)
    for (int s = 0; s < NSH; s += 2) {
        RSD_STEP(true);
        RSD_STEP(s + 2 < NSH);
    }
#undef RSD_WAIT
#undef RSD_STEP
#undef RSD_MAC
#undef RSD_F
    if (sh > 0) {
#pragma unroll
        for (int l = 0; l < NL; ++l)
#pragma unroll
            for (int i = 0; i < KPL; ++i) s_part[sh - 1][l][i][lane] = acc[l][i];
    }
    __syncthreads();
    if (sh > 0) return;
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            double a = acc[l][i];
#pragma unroll
            for (int q = 0; q < SH - 1; ++q) a += s_part[q][l][i][lane];
            if (k[i] < Nk && k[i] >= Nklow) T[(((size_t)w * NL + l) * NROW) * Nk + k[i]] += k2[i] * a;
        }
}

// The same scheme for Nl = 2 (NIR = 8, Na = 2): the polynomials have degree 7, so the monomials of t = z / RS_ZS are the basis
// (V8 = identity); the 8 (a, l, l') blocks x 4 slots are 32 rows = two row tiles: tile tau <-> l' = tau, lane group jg <-> (a, l) =
// (1, 0), (1, 1), (0, 0), (0, 1); slots 0 -> (v = l', half 0), 1, 2 -> (v = slot - 1, half 1), 3 -> empty.  Four MFMAs per step, every
// output row owned by one lane group, no cross-lane traffic.
__global__ __launch_bounds__(256, 2)
void resum_mfma2_kernel(int Nk, int Nklow, int schunk, const double* __restrict__ kk,
                                                             const double* __restrict__ H, const double* __restrict__ V8,
                                                             const double* __restrict__ RSA, const double* __restrict__ RSC,
                                                             const double* __restrict__ l11, const double* __restrict__ lct,
                                                             double* __restrict__ T, double* __restrict__ part, int nsplit) {
    constexpr int NL = 2, NT = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int jg = lane >> 4, n = lane & 15;
    const int k = Nklow + (blockIdx.x * 4 + wave) * 16 + n, w = blockIdx.y, split = blockIdx.z;
    const bool live = k < Nk;
    const int kc = live ? k : Nk - 1;
    const double k2 = kk[kc] * kk[kc];
    // B operand: the monomials t^jg and t^(jg + 4) of this lane's point (V8 is the identity for Nl = 2: nothing to evaluate)
    auto powers = [&](double t, double& p0, double& p1) {
        const double t2 = t * t;
        p0 = jg == 0 ? 1.0 : (jg == 1 ? t : (jg == 2 ? t2 : t2 * t));
        p1 = p0 * (t2 * t2);
    };
    double aop[NT][2];
#pragma unroll
    for (int tau = 0; tau < NT; ++tau)
#pragma unroll
        for (int t = 0; t < 2; ++t) aop[tau][t] = RSA[((size_t)w * RS_ROWS + 16 * tau + n) * RS_NB + jg + 4 * t];
    double accL[12], accCt[NT], acc11[NT];
#pragma unroll
    for (int i = 0; i < 12; ++i) accL[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) accCt[i] = acc11[i] = 0.0;
    const int s0 = split * schunk, s1 = min(NS, s0 + schunk);
    const double* ct = RSC + ((size_t)w * NS + s0) * RS_REC;
    double h[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) h[v] = H[((size_t)v * NS + s0) * Nk + kc];
    double z = k2 * ct[42], y = k2 * ct[43];
    double b0, b1;
    powers(z * (1.0 / RS_ZS), b0, b1);
#pragma unroll
    for (int tau = 0; tau < NT; ++tau)
#pragma unroll
        for (int t = 0; t < 2; ++t) asm volatile("" : "+v"(aop[tau][t]));
    for (int s = s0; s < s1; ++s) {
        const int sn = s + 1 < s1 ? s + 1 : s;
        const double* ctn = RSC + ((size_t)w * NS + sn) * RS_REC;
        double cv[14 * NT];
#pragma unroll
        for (int i = 0; i < 14 * NT; ++i) cv[i] = ct[i];
        const double xn = ctn[42], yn0 = ctn[43];
        double hn[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) hn[v] = H[((size_t)v * NS + sn) * Nk + kc];
        __builtin_amdgcn_sched_barrier(0);
        v4d D[NT];
#pragma unroll
        for (int tau = 0; tau < NT; ++tau) D[tau] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[tau][0], b0, (v4d){0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
#pragma unroll
        for (int tau = 0; tau < NT; ++tau) D[tau] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[tau][1], b1, D[tau], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        const double zn = k2 * xn, yn = k2 * yn0;
        double bn0, bn1;
        powers(zn * (1.0 / RS_ZS), bn0, bn1);
        const double zh[2] = {z * h[0], z * h[1]}, yh[2] = {y * h[0], y * h[1]};
#pragma unroll
        for (int tau = 0; tau < NT; ++tau) {
            const double W = fma(zh[tau], D[tau][0], fma(yh[0], D[tau][1], yh[1] * D[tau][2]));
            acc11[tau] = fma(W, cv[tau * 14], acc11[tau]);          // every lane accumulates both roles; only its own is read
            accCt[tau] = fma(W, cv[tau * 14 + 1], accCt[tau]);
#pragma unroll
            for (int i = 0; i < 12; ++i) accL[i] = fma(W, cv[tau * 14 + 2 + i], accL[i]);
        }
        __builtin_amdgcn_sched_barrier(0);
        ct = ctn;
        z = zn;
        y = yn;
        b0 = bn0;
        b1 = bn1;
        h[0] = hn[0];
        h[1] = hn[1];
    }
    if (!live) return;
    const int l = jg & 1;  // multipole of this lane group's block
    double o18[18], oA[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) o18[i] = lct[i] * accCt[0] + lct[6 + i] * accCt[1];
#pragma unroll
    for (int i = 0; i < 12; ++i) o18[6 + i] = accL[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) oA[i] = l11[i] * acc11[0] + l11[3 + i] * acc11[1];
    if (nsplit == 1) {
        double* dst = T + (((size_t)w * NL + l) * NROW) * Nk + k;
        if (jg < 2) {
#pragma unroll
            for (int i = 0; i < 18; ++i) dst[(size_t)(3 + i) * Nk] += o18[i];
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) dst[(size_t)i * Nk] += oA[i];
        }
    } else {  // partial sums over the s slices, added in a fixed order by resum_sum_kernel
        double* pw = part + (((size_t)w * nsplit + split) * NL + l) * 21 * Nk + k;
        if (jg < 2) {
#pragma unroll
            for (int i = 0; i < 18; ++i) pw[(size_t)(3 + i) * Nk] = o18[i];
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) pw[(size_t)i * Nk] = oA[i];
        }
    }
}

__global__ __launch_bounds__(256) void resum_sum_kernel(int Nk, int Nl, int nchunk, const double* __restrict__ part,
                                                        double* __restrict__ T) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y % 21, l = blockIdx.y / 21, w = blockIdx.z;
    if (k >= Nk) return;
    double a = 0.0;
    for (int c = 0; c < nchunk; ++c) a += part[((((size_t)w * nchunk + c) * Nl + l) * 21 + i) * Nk + k];
    T[(((size_t)w * Nl + l) * NROW + i) * Nk + k] += a;
}

// ------------------------------------------------------------------------------------------------
// AP: not-a-knot cubic spline of every template row, then for each (row, k): P(k', mu') = sum_l'
// spline_l'(k') L_l'(mu'), projected back on (2l+1)/2 L_l(mu) with the trapezoid rule on linspace(0,1,nmu)
// (reference pybird.py:1581-1621).
//
// spline_kernel: the knot derivatives are  s = A^-1 R y  with A the (constant) not-a-knot tridiagonal matrix;
// A^-1 R decays like 0.27^|i-j|, so the host ships it as a band of half-width SPL_HB (truncation < 1e-18,
// checked in tests) and the solve becomes a banded matrix product.  Output: S[series][i] = s_i; together with y_i = T[series][i]
// that is the Hermite data of the piecewise cubic on [k_i, k_i+1] (round 3: the knot values are no longer copied beside the slopes --
// 37 MB less written per step; the consumers read y from the template block itself).
// ------------------------------------------------------------------------------------------------
constexpr int SPL_HB = 32;

// Matrix-core form: S[series][i] = sum_j y[series][j] BandT[j][i] with the band as the (register-resident) B operand.
// Workgroup = 4 waves = 64 knots; wave q owns the 16-knot tile i0 + 16 q and needs the inputs j in [tile - 32, tile + 48): 20
// K-steps whose 20 B fragments are loaded once and reused for every series.  The y window of 16 series x 128 knots goes
// through LDS (register-prefetched one group ahead); one group of 16 series = 20 MFMAs per wave.
constexpr int SPL_W = 128, SPL_LD = SPL_W + 2;  // staged window (64 knots + 2 x 32 halo), LDS row stride (conflict-free b64 reads)

// (register cap: 96 in all instead of 96 + 8 accumulator registers -- what is free beside two resummation waves on a SIMD; same speed alone)
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(88))) void spline_kernel(int Nk, int nseries, int rlo, int rsel, const double* __restrict__ T, const double* __restrict__ band,
                                                     double* __restrict__ S) {
    __shared__ double ys[16 * SPL_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    int ktile, share;  // the k tiles of one share of the series run on one XCD: their halo windows overlap by half
    xcd_decode((Nk + 63) / 64, ktile, share);
    const int nshare = gridDim.x / ((Nk + 63) / 64);
    const int w0 = ktile * 64 - SPL_HB;      // first knot of the staged window
    const int it0 = ktile * 64 + 16 * wave;  // this wave's output tile
    // B fragments: K-step t, lane (g, r): weight of input j = it0 - 32 + 4 t + g for output knot i = it0 + r, i.e. band[d][i], d = 4 t + g - r
    double bf[20];
#pragma unroll
    for (int t = 0; t < 20; ++t) {
        const int d = 4 * t + g - r, i = it0 + r;
        bf[t] = (d >= 0 && d <= 2 * SPL_HB && i < Nk) ? band[(size_t)d * Nk + i] : 0.0;
    }
    const int ngroups = (nseries + 15) / 16;
    const int per = (ngroups + nshare - 1) / nshare;
    const int g0 = share * per, g1 = min(ngroups, g0 + per);
    // staging: 16 series x 128 knots = 2048 values, 8 per thread (series = e / 128, knot = e % 128: coalesced rows)
    // nseries counts the selected series: rows [rlo, rlo + rsel) of every (cosmology, l) block of NROW (rsel = NROW: all of them)
    auto row_of = [&](int sp) { return rsel == NROW ? sp : (sp / rsel) * NROW + rlo + sp % rsel; };  // (uniform branch: no division on the headline path)
    double pre[8];
    auto fetch = [&](int grp) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u, sr = e >> 7, jj = w0 + (e & 127), series = grp * 16 + sr;
            pre[u] = (series < nseries && jj >= 0 && jj < Nk) ? T[(size_t)row_of(series) * Nk + jj] : 0.0;
        }
    };
    if (g0 < g1) fetch(g0);
    for (int grp = g0; grp < g1; ++grp) {
        __syncthreads();  // the previous group's window has been consumed
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u;
            ys[(e >> 7) * SPL_LD + (e & 127)] = pre[u];
        }
        __syncthreads();
        if (grp + 1 < g1) fetch(grp + 1);
        v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
        const double* yr = ys + r * SPL_LD + 16 * wave + g;  // A operand: series r, input j = it0 - 32 + 4 t + g -> window offset 16 wave + 4 t + g
#pragma unroll
        for (int t = 0; t < 20; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(yr[4 * t], bf[t], acc, 0, 0, 0);
        // D: rows (series) g + 4 q, column (knot) r
        const int i = it0 + r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int sr = g + 4 * q, series = grp * 16 + sr;
            if (series < nseries && i < Nk) S[(size_t)row_of(series) * Nk + i] = acc[q];
        }
    }
}

__device__ __forceinline__ int bspl_first(int i, int Nk) { return min(max(i - 1, 0), Nk - 4); }  // J_i of tables.bspline_tables

__device__ inline int knot_interval(const double* __restrict__ kk, int Nk, double x) {
    int lo = 0, hi = Nk - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (kk[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------
// AP as prefix sums over mu (ap_prefix_kernel) + interval moments by differences (ap_weights_kernel).
// With k' = kq (1 + rho_j), kq = k / qperp, rho_j = sqrt(1 + g mu_j^2) - 1, the offset inside knot interval i is
//     t_j = k' - k_i = kq rho_j + delta,   delta = kq - k_i,
// so the moments of the quadrature on the nodes [ja, jb) that fall into interval i,
//     M_i[l][l'][p] = sum_{j in [ja, jb)} wl[l][j] lp[l'][j] t_j^p = sum_{q <= p} C(p,q) kq^q delta^(p-q) (PS[jb] - PS[ja])[l'][l][q],
// need only the k-independent prefix sums  PS[w][j][l'][l][q] = sum_{j' < j} wl[l][j'] lp[l'][j'] rho_j'^q  (one small
// table per cosmology) and the node indices where k'(mu) crosses the knots (closed form + a one-step fix-up against the
// stored roots, so every node lands in the interval the comparison k_i <= k' < k_i+1 selects).  Then
//     out[l][row][k] = sum_i sum_{l',p} M_i[l][l'][p] CO[l'][row][i][p],
// i.e. per (k, row, l) the nmu cubic evaluations of the direct form (reference pybird.py:1581-1621) collapse to
// (intervals crossed, ~3) x 4 NL FMAs.  No mu loop, no LDS, no divergence beyond the number of intervals crossed.
// ------------------------------------------------------------------------------------------------
template <int NL>
__global__ __launch_bounds__(320) void ap_prefix_kernel(int nmu, const double* __restrict__ DAw, const double* __restrict__ Hw,
                                                        const double* __restrict__ fid, const double* __restrict__ mu,
                                                        const double* __restrict__ wmu, const double* __restrict__ legmu,
                                                        double* __restrict__ PS, double* __restrict__ ROOT) {
    // sequences (l', l, q), chunks of the mu range per sequence: NS x NCH threads (seven chunks on 256 threads measured 31 instead of 20 us)
    constexpr int NS = NL * NL * 4, NCH = 8;
    extern __shared__ double sm[];
    double* s_rho = sm;                    // [nmu]
    double* s_lp = sm + nmu;               // [NL][nmu]  L_l'(mu')
    double* s_wl = sm + (1 + NL) * nmu;    // [NL][nmu]  wmu (2l+1)/2 L_l(mu)
    double* s_tot = sm + (1 + 2 * NL) * nmu;  // [NS][NCH] chunk totals -> chunk offsets
    const int w = blockIdx.x;
    const double qperp = DAw[w] / fid[0], qpar = fid[1] / Hw[w];
    const double F = qpar / qperp, g = 1.0 / (F * F) - 1.0;
    for (int j = threadIdx.x; j < nmu; j += blockDim.x) {
        const double m = mu[j];
        const double root = sqrt(1.0 + m * m * g);
        const double mp = m / (F * root), x2 = mp * mp;
        ROOT[(size_t)w * nmu + j] = root;
        s_rho[j] = g * m * m / (1.0 + root);
        s_lp[j] = 1.0;
        s_lp[nmu + j] = 0.5 * (3.0 * x2 - 1.0);
        if (NL > 2) s_lp[2 * nmu + j] = (35.0 * x2 * x2 - 30.0 * x2 + 3.0) * 0.125;
#pragma unroll
        for (int l = 0; l < NL; ++l) s_wl[l * nmu + j] = wmu[j] * legmu[l * nmu + j];
    }
    __syncthreads();
    const int seq = threadIdx.x % NS, ch = threadIdx.x / NS;
    const int q = seq & 3, l = (seq >> 2) % NL, lp = seq / (4 * NL);
    const int clen = (nmu + NCH - 1) / NCH, j0 = ch * clen, j1 = min(nmu, j0 + clen);
    double* ps = PS + (size_t)w * (nmu + 1) * NS + seq;
    // two sweeps over the chunk from LDS: totals first, then -- once the chunk offsets are known -- the running sums, written once (round 2
    // wrote chunk-local sums to global memory and came back to add the offsets: a global read-modify-write in the middle of a 20 us kernel)
    auto term = [&](int j) {
        const double r = s_rho[j];
        const double rq = q == 0 ? 1.0 : (q == 1 ? r : (q == 2 ? r * r : r * r * r));
        return s_wl[l * nmu + j] * s_lp[lp * nmu + j] * rq;
    };
    if (ch < NCH) {
        double s = 0.0;
        for (int j = j0; j < j1; ++j) s += term(j);
        s_tot[seq * NCH + ch] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS) {  // exclusive scan of the chunk totals
        double run = 0.0;
        for (int c = 0; c < NCH; ++c) {
            const double t = s_tot[threadIdx.x * NCH + c];
            s_tot[threadIdx.x * NCH + c] = run;
            run += t;
        }
        PS[(size_t)w * (nmu + 1) * NS + threadIdx.x] = 0.0;
    }
    __syncthreads();
    if (ch < NCH) {
        double s = s_tot[seq * NCH + ch];
        for (int j = j0; j < j1; ++j) {
            s += term(j);
            ps[(size_t)(j + 1) * NS] = s;
        }
    }
}

// ap_direct_kernel: the stage in the reference's own form (pybird.py:1581-1621) -- per (k, row) the nmu nodes are walked in order, the
// spline is evaluated at k'(mu_j) in the interval the comparison k_i <= k' < k_i+1 selects (end intervals extrapolate), weighted with
// L_l'(mu'_j) and projected on (2l+1)/2 L_l(mu_j) with the trapezoid weights.  It is the FALLBACK of the two-kernel form below for tiles
// whose distortion crosses more knot intervals than the fast path keeps (META flag), and the whole stage with EFTB_AP_MODE=2: small
// (no LDS, few registers), so that its launch never waits for resources when every workgroup just reads its flag and leaves.
// Workgroup = one wave = 64 k of one cosmology, the thread walks the template rows one after the other (a light launch: 1 024 waves at
// Nk = 512, B = 128 -- the gate must not wait for resources beside the resummation kernel); rows >= nr (Pstl unless APst) are copied through.
// BSPL: S holds the B-spline coefficients of the rows (the fast path's spline data, tables.bspline_tables; LOCAL = its per-interval matrices)
// instead of the knot slopes of the Hermite form.
template <int NL, bool BSPL>
__global__ __launch_bounds__(64) void ap_direct_kernel(int Nk, int nmu, int rlo, int nr, const double* __restrict__ kk, const double* __restrict__ DAw,
                                                       const double* __restrict__ Hw, const double* __restrict__ fid,
                                                       const double* __restrict__ mu, const double* __restrict__ wmu,
                                                       const double* __restrict__ legmu, const double* __restrict__ ROOT,
                                                       const double* __restrict__ T, const double* __restrict__ S, double* __restrict__ Tout,
                                                       const int4* __restrict__ META, const double* __restrict__ bias, double* __restrict__ Plk,
                                                       double* __restrict__ PlkHost, int msplit, int* __restrict__ nonfinite,
                                                       const double* __restrict__ LOCAL) {
    const int KT = (Nk + 63) / 64;
    int kt, w;
    xcd_decode(KT, kt, w);
    // fallback duty only: the 32-k tile of this lane went through ap_rows_kernel (the gate is per half wave; no barrier below)
    if (META && !META[(size_t)w * 2 * KT + 2 * kt + (threadIdx.x >> 5)].w) return;
    const int k = kt * 64 + threadIdx.x;
    if (k >= Nk) return;
    const double qperp = DAw[w] / fid[0], qpar = fid[1] / Hw[w], F = qpar / qperp;
    const double kq = kk[k] / qperp, c = 2.0 / (qperp * qperp * qpar);
    const double* root = ROOT + (size_t)w * nmu;
    const int i_first = knot_interval(kk, Nk, kq * root[0]);
    // bias contraction riding along (bias != null): two FMA chains, rows [0, msplit) and [msplit, NROW), added at the end -- the order
    // of reduce_kernel and of ap_rows_kernel's epilogue, so that a fallback tile's P_l is bit-identical to theirs
    double ch0[NL], ch1[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) ch0[l] = ch1[l] = 0.0;
    const double* bw = bias ? bias + (size_t)w * NROW : nullptr;
    for (int r = 0; r < NROW; ++r) {
        const double br = bw ? bw[r] : 0.0;
        if (r >= nr || r < rlo) {  // rows outside [rlo, nr) are copied through
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const size_t o = (((size_t)w * NL + l) * NROW + r) * Nk + k;
                const double v = T[o];
                Tout[o] = v;
                if (r < msplit) ch0[l] = fma(br, v, ch0[l]); else ch1[l] = fma(br, v, ch1[l]);
            }
            continue;
        }
        const size_t rbase = ((size_t)w * NL * NROW + r) * Nk;
        double acc[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) acc[l] = 0.0;
        int i = i_first;
        for (int j = 0; j < nmu; ++j) {
            const double rt = root[j], kp = kq * rt;
            while (i < Nk - 2 && kk[i + 1] <= kp) ++i;
            while (i > 0 && kk[i] > kp) --i;
            const double klo = kk[i], h = kk[i + 1] - klo, ih = 1.0 / h, t = kp - klo;
            const double m = mu[j], mp = m / (F * rt), x2 = mp * mp;
            const double lpv[3] = {1.0, 0.5 * (3.0 * x2 - 1.0), (35.0 * x2 * x2 - 30.0 * x2 + 3.0) * 0.125};
            double P = 0.0;
            if (BSPL) {
                // value of the four basis pieces of interval i at t: sum_p local[i][e][p] t^p; the spline is their combination with c[J_i + e]
                const double4* lc = reinterpret_cast<const double4*>(LOCAL + (size_t)i * 16);
                double be[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double4 n4 = lc[e];
                    be[e] = fma(fma(fma(n4.w, t, n4.z), t, n4.y), t, n4.x);
                }
                const int J = bspl_first(i, Nk);
#pragma unroll
                for (int lp = 0; lp < NL; ++lp) {
                    const double* cp = S + rbase + (size_t)lp * NROW * Nk + J;
                    P = fma(fma(be[0], cp[0], fma(be[1], cp[1], fma(be[2], cp[2], be[3] * cp[3]))), lpv[lp], P);
                }
            } else {
#pragma unroll
                for (int lp = 0; lp < NL; ++lp) {
                    const size_t o = rbase + (size_t)lp * NROW * Nk + i;
                    const double ya = T[o], yb = T[o + 1], sa = S[o], sb = S[o + 1];
                    const double sl = (yb - ya) * ih;
                    const double c3 = (sa + sb - 2.0 * sl) * ih * ih;
                    const double c2 = (sl - sa) * ih - c3 * h;
                    P = fma(fma(fma(fma(c3, t, c2), t, sa), t, ya), lpv[lp], P);
                }
            }
            const double wj = wmu[j] * P;
#pragma unroll
            for (int l = 0; l < NL; ++l) acc[l] = fma(wj, legmu[(size_t)l * nmu + j], acc[l]);
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const double v = c * acc[l];
            Tout[(((size_t)w * NL + l) * NROW + r) * Nk + k] = v;
            if (r < msplit) ch0[l] = fma(br, v, ch0[l]); else ch1[l] = fma(br, v, ch1[l]);
        }
    }
    if (bias) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const double a = ch0[l] + ch1[l];
            Plk[((size_t)w * NL + l) * Nk + k] = a;
            if (PlkHost) PlkHost[((size_t)w * NL + l) * Nk + k] = a;
            if (nonfinite && !(fabs(a) <= 1.79769313486231570815e308)) atomicMax(nonfinite, w + 1);
        }
    }
}

// ap_moments_kernel (the round-1 form of the stage, kept for fine k grids: at Nk = 2048 a 2 % distortion crosses ~45 knots, more than the
// weight tables of the fast path hold per k, and every tile would fall back to the node-by-node quadrature of ap_direct_kernel).  The interval
// moments are binomial combinations of the mu prefix sums of ap_prefix_kernel taken at the node indices where k'(mu) crosses the knots, so a
// (row, k, l) costs 12 FMAs per interval crossed instead of a 200-node loop.
// Workgroup = 64 k x 4 waves of one cosmology; wave <-> interval slot (s = wave, wave + 4, ...), so
// the intervals that k'(mu) crosses are handled in parallel: slot s of a k is interval i = i_first + s dir, and its
// node range [ja, jb) comes from the closed-form crossings of its two knots (the same function of (kq, knot) in both
// neighbouring slots, so the ranges tile [0, nmu) exactly).  Knots and roots sit in LDS; the four waves' partial sums
// are added through LDS in a fixed order.
template <int NL, int NR, int RS>
__global__ __launch_bounds__(256, 2) void ap_moments_kernel(int Nk, int nmu, const double* __restrict__ kk, const double* __restrict__ DAw,
                                                       const double* __restrict__ Hw, const double* __restrict__ fid,
                                                       const double* __restrict__ mu, const double* __restrict__ PS,
                                                       const double* __restrict__ ROOT, const double* __restrict__ T,
                                                       const double* __restrict__ S, double* __restrict__ Tout) {
    constexpr int NS = NL * NL * 4;
    constexpr int NRT = (NR + RS - 1) / RS;  // rows per lane: the NR rows are split over RS workgroups (blockIdx.z)
    constexpr int NACC = NL * NRT;
    extern __shared__ double sm[];
    double* s_k = sm;               // [Nk]
    double* s_root = sm + Nk;       // [nmu]
    double* red = sm + Nk + nmu;    // [4][NACC][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane, w = blockIdx.y, rbase = blockIdx.z * NRT;
    for (int e = threadIdx.x; e < Nk; e += 256) s_k[e] = kk[e];
    for (int e = threadIdx.x; e < nmu; e += 256) s_root[e] = ROOT[(size_t)w * nmu + e];
    __syncthreads();
    const double qperp = DAw[w] / fid[0], qpar = fid[1] / Hw[w];
    const double F = qpar / qperp, g = 1.0 / (F * F) - 1.0;
    const bool live = k < Nk;
    const double kq = s_k[live ? k : Nk - 1] / qperp;
    const double inv_kq = 1.0 / kq, inv_g = 1.0 / g;
    const double* ps = PS + (size_t)w * (nmu + 1) * NS;
    const bool up = g > 0.0;  // k'(mu) rises or falls with mu
    const int dir = up ? 1 : -1;
    const double jscale = (nmu - 1) / mu[nmu - 1];  // node index per unit mu (uniform grid: only a first guess, see the fix-up)
    double acc[NL][NRT];
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int r = 0; r < NRT; ++r) acc[l][r] = 0.0;
    // first node that lies past knot kb (k'_j >= kb when rising, k'_j < kb when falling)
    auto cross = [&](double kb) -> int {
        const double rc = kb * inv_kq, x = (rc * rc - 1.0) * inv_g;  // mu^2 at the crossing (a seed: the fix-up below decides)
        int j = nmu;
        if (x >= 0.0 && x < 1.0) j = (int)(sqrt(x) * jscale) + 1;
        j = max(0, min(j, nmu));
        while (j > 0 && (up ? kq * s_root[j - 1] >= kb : kq * s_root[j - 1] < kb)) --j;
        while (j < nmu && !(up ? kq * s_root[j] >= kb : kq * s_root[j] < kb)) ++j;
        return j;
    };
    const int i_first = knot_interval(s_k, Nk, kq * s_root[0]);
    const int i_last = knot_interval(s_k, Nk, kq * s_root[nmu - 1]);
    const int nslot = live ? (up ? i_last - i_first : i_first - i_last) + 1 : 0;
    for (int s = wave; s < nslot; s += 4) {
        const int i = i_first + s * dir;
        const double klo = s_k[i], khi = s_k[i + 1];
        const int ja = s == 0 ? 0 : cross(up ? klo : khi);
        const int jb = s == nslot - 1 ? nmu : cross(up ? khi : klo);
        if (jb <= ja) continue;
        const double h = khi - klo, ih = 1.0 / h;
        const double dl = kq - klo, dl2 = dl * dl, a2 = kq * kq;
        const double c10 = dl, c11 = kq, c20 = dl2, c21 = 2.0 * kq * dl, c22 = a2;
        const double c30 = dl2 * dl, c31 = 3.0 * kq * dl2, c32 = 3.0 * a2 * dl, c33 = a2 * kq;
        const double* pa = ps + (size_t)ja * NS;
        const double* pb = ps + (size_t)jb * NS;
        const size_t cw = (size_t)w * NL * NROW * Nk + i;  // knot i of series (l' = 0, row 0): y in T, s in S
        // memory round trips are what this kernel waits for (PMC: 75 % of the wave cycles): the prefix sums of all l' are
        // fetched in one batch, and the spline data of l' + 1 is in flight while l' is being accumulated
        double ms[NL][NL][4];
        {
            double4 a4[NL][NL], b4[NL][NL];
#pragma unroll
            for (int lp = 0; lp < NL; ++lp)
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    b4[lp][l] = *reinterpret_cast<const double4*>(pb + (lp * NL + l) * 4);
                    a4[lp][l] = *reinterpret_cast<const double4*>(pa + (lp * NL + l) * 4);
                }
#pragma unroll
            for (int lp = 0; lp < NL; ++lp)
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    const double d0 = b4[lp][l].x - a4[lp][l].x, d1 = b4[lp][l].y - a4[lp][l].y;
                    const double d2 = b4[lp][l].z - a4[lp][l].z, d3 = b4[lp][l].w - a4[lp][l].w;
                    ms[lp][l][0] = d0;
                    ms[lp][l][1] = fma(c10, d0, c11 * d1);
                    ms[lp][l][2] = fma(c20, d0, fma(c21, d1, c22 * d2));
                    ms[lp][l][3] = fma(c30, d0, fma(c31, d1, fma(c32, d2, c33 * d3)));
                }
        }
        double2 ya[2][NRT], yb[2][NRT];
        auto fetch = [&](int lp, int buf) {
#pragma unroll
            for (int r = 0; r < NRT; ++r) {
                const size_t o = cw + ((size_t)lp * NROW + min(rbase + r, NR - 1)) * Nk;
                ya[buf][r] = make_double2(T[o], S[o]);          // (y_i, s_i)
                yb[buf][r] = make_double2(T[o + 1], S[o + 1]);  // (y_i+1, s_i+1)
            }
        };
        fetch(0, 0);
#pragma unroll
        for (int lp = 0; lp < NL; ++lp) {
            if (lp + 1 < NL) fetch(lp + 1, (lp + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch above the arithmetic that consumes the previous buffer
#pragma unroll
            for (int r = 0; r < NRT; ++r) {
                const double2 ca = ya[lp & 1][r], cb = yb[lp & 1][r];  // -> power form on [k_i, k_i+1]
                const double sl = (cb.x - ca.x) * ih;
                const double c3 = (ca.y + cb.y - 2.0 * sl) * ih * ih;
                const double c2 = (sl - ca.y) * ih - c3 * h;
#pragma unroll
                for (int l = 0; l < NL; ++l)
                    acc[l][r] = fma(ms[lp][l][0], ca.x, fma(ms[lp][l][1], ca.y, fma(ms[lp][l][2], c2, fma(ms[lp][l][3], c3, acc[l][r]))));
            }
        }
    }
    // sum the four waves in a fixed order and write
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int r = 0; r < NRT; ++r) red[(wave * NACC + l * NRT + r) * 64 + lane] = acc[l][r];
    __syncthreads();
    const double c = 2.0 / (qperp * qperp * qpar);
    for (int e = wave; e < NACC; e += 4) {
        const int l = e / NRT, r = e % NRT;
        const double v = (red[(0 * NACC + e) * 64 + lane] + red[(1 * NACC + e) * 64 + lane]) + (red[(2 * NACC + e) * 64 + lane] + red[(3 * NACC + e) * 64 + lane]);
        if (live && rbase + r < NR) Tout[(((size_t)w * NL + l) * NROW + rbase + r) * Nk + k] = c * v;
    }
    constexpr int NCP = NROW - NR > 0 ? NROW - NR : 1;  // rows that APeffect leaves alone (Pstl unless APst)
    if (live && NR < NROW && blockIdx.z == 0)
        for (int e = wave; e < NCP * NL; e += 4) {
            const int l = e / NCP, r = NR + e % NCP;
            const size_t o = (((size_t)w * NL + l) * NROW + r) * Nk + k;
            Tout[o] = T[o];
        }
}

// ------------------------------------------------------------------------------------------------
// AP, two-kernel form (the default path; ap_direct_kernel above is the fallback for distortions that cross more knot
// intervals than the fast path keeps).  The stage is LINEAR in the spline data: for one cosmology and one output k
//     out[l][row][k] = c sum_{l'} sum_{d} ( Wy[l'][l][d] y[l'][row][i0 + d] + Ws[l'][l][d] s[l'][row][i0 + d] ),
// where (y, s) are the knot values / derivatives written by spline_kernel, i0 = i0(w, k) the lowest knot interval k'(mu) visits and
// the knot weights follow from the interval moments M_i (header above ap_prefix_kernel) by inserting the Hermite form of the cubic:
//     c0 = y_i, c1 = s_i, c2 = (3 sl - 2 s_i - s_i+1) / h, c3 = (s_i + s_i+1 - 2 sl) / h^2, sl = (y_i+1 - y_i) / h   =>
//     left knot :  Wy += m0 - 3 m2 / h^2 + 2 m3 / h^3,   Ws += m1 - 2 m2 / h + m3 / h^2
//     right knot:  Wy += 3 m2 / h^2 - 2 m3 / h^3,        Ws += - m2 / h + m3 / h^2            (m_p = M_i[l][l'][p]).
// The weights depend on (DA, H) only -- inputs -- so ap_weights_kernel runs on the look-ahead stream with the prefix sums, off the
// critical path; what is left behind the resummation is ap_rows_kernel, a banded product that streams the spline data once
// through LDS: 66 MB in, 33 MB out, a few dozen FMAs per output.
//   ap_weights_kernel  workgroup = 64 k x NL waves of one cosmology; wave <-> l', the thread walks its k's intervals in mu order carrying
//                      the shared knot's contribution; writes, per tile of 32 k (a half wave), W[w][tile][d][l][l'][{y,s}][32], i0[w][k] and
//                      the tile's window (lowest knot, span, knots per k); tiles that need more than APW_DCAP knots per k or a window
//                      of more than APW_WIN knots are flagged and left to ap_direct_kernel
//   ap_rows_kernel     workgroup = (tile of 32 k, cosmology) x NL waves, wave <-> output multipole l, the two half waves <-> two halves of
//                      the template rows.  The (y, s) window of ALL rows and all l' sits in LDS (two planes, filled by global_load_lds with no
//                      register staging), so every byte of the weights, of the templates and of the slopes is read from HBM once
//                      (round 2 walked the rows in chunks of 7 and re-read the 44 MB of weights per chunk: 199 MB fetched for 110 needed);
//                      when REDUCE follows directly, the bias contraction P_l = sum_row b_row out[l][row] rides in the epilogue.
// ------------------------------------------------------------------------------------------------
constexpr int APW_DCAP = 32;  // knots per k on the fast path
#ifndef APR_AHEAD
#define APR_AHEAD 6
#endif
constexpr int APW_WIN = 64;   // LDS window of a 32-k tile, in knots (32 k + the drift of i0 across the tile + the knots per k)

template <int NL>
__global__ __launch_bounds__(64 * NL) void ap_weights_kernel(int Nk, int nmu, const double* __restrict__ kk, const double* __restrict__ DAw,
                                                         const double* __restrict__ Hw, const double* __restrict__ fid,
                                                         const double* __restrict__ mu, const double* __restrict__ PS,
                                                         const double* __restrict__ ROOT, const double* __restrict__ LOCAL,
                                                         double* __restrict__ W, int* __restrict__ I0, int4* __restrict__ META) {
    // NL waves, NL (l', l) pairs each (wave <-> l', the order of the prefix sums): every wave walks the same interval slots, so fewer waves
    // means fewer copies of the crossing arithmetic, and the pairs divide evenly
    constexpr int NS = NL * NL * 4, NP = NL * NL, PPW = NL, NT = 64 * NL;  // prefix sequences, (l', l) pairs, pairs per wave, threads
    extern __shared__ double sm[];
    double* s_k = sm;                   // [Nk]
    double* s_root = sm + Nk;           // [nmu]
    __shared__ int s_red[2][3];         // per half wave (= tile of 32 k): min first coefficient, max first coefficient, max coefficients per k
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hw = lane >> 5;
    const int KT = (Nk + 63) / 64;
    int kt, w;
    xcd_decode(KT, kt, w);
    const int k = kt * 64 + lane;
    for (int e = threadIdx.x; e < Nk; e += NT) s_k[e] = kk[e];
    for (int e = threadIdx.x; e < nmu; e += NT) s_root[e] = ROOT[(size_t)w * nmu + e];
    if (threadIdx.x < 2) {
        s_red[threadIdx.x][0] = 0x7fffffff;
        s_red[threadIdx.x][1] = 0;
        s_red[threadIdx.x][2] = 0;
    }
    __syncthreads();
    const double qperp = DAw[w] / fid[0], qpar = fid[1] / Hw[w];
    const double F = qpar / qperp, g = 1.0 / (F * F) - 1.0;
    const bool live = k < Nk;
    const double kq = s_k[live ? k : Nk - 1] / qperp;
    const double inv_kq = 1.0 / kq, inv_g = 1.0 / g;  // (the closed form only seeds the crossing: the fix-up below decides against the stored roots)
    // the cosmology's prefix sums (58 KB) are gathered from the L2 / L1: staged in LDS they left room for two workgroups per CU, and the kernel
    // measured 80 instead of 56 us
    const double* ps = PS + (size_t)w * (nmu + 1) * NS;
    const bool up = g > 0.0;
    const int dir = up ? 1 : -1;
    const double jscale = (nmu - 1) / mu[nmu - 1];
    // first node that lies past knot kb (k'_j >= kb when rising, k'_j < kb when falling): closed form + a one-step fix-up against the stored roots
    auto cross = [&](double kb) -> int {
        const double rc = kb * inv_kq, x = (rc * rc - 1.0) * inv_g;
        int j = nmu;
        if (x >= 0.0 && x < 1.0) j = (int)(sqrt(x) * jscale) + 1;
        j = max(0, min(j, nmu));
        while (j > 0 && (up ? kq * s_root[j - 1] >= kb : kq * s_root[j - 1] < kb)) --j;
        while (j < nmu && !(up ? kq * s_root[j] >= kb : kq * s_root[j] < kb)) ++j;
        return j;
    };
    const int i_first = knot_interval(s_k, Nk, kq * s_root[0]);
    const int i_last = knot_interval(s_k, Nk, kq * s_root[nmu - 1]);
    const int nslot = (up ? i_last - i_first : i_first - i_last) + 1;
    // B-spline coefficients this k touches: [jlow, jlow + nD), four per interval (tables.bspline_tables)
    const int jlow = bspl_first(min(i_first, i_last), Nk), nD = live ? bspl_first(max(i_first, i_last), Nk) + 4 - jlow : 0;
    if (wave == 0) {
        if (live) {
            I0[(size_t)w * KT * 64 + k] = jlow;
            atomicMin(&s_red[hw][0], jlow);
            atomicMax(&s_red[hw][1], jlow);
            atomicMax(&s_red[hw][2], nD);
        } else {
            I0[(size_t)w * KT * 64 + k] = -1;  // resolved to the tile's lowest coefficient by the consumer
        }
    }
    __syncthreads();
    const int jmin = s_red[hw][0], D = s_red[hw][2], span = s_red[hw][1] - jmin + D;
    const bool fallback = D > APW_DCAP || span > APW_WIN;  // (a tile with no k inside the grid: D = 0, never read)
    if ((threadIdx.x & 31) == 0 && wave == 0) META[(size_t)w * 2 * KT + 2 * kt + hw] = make_int4(jmin, span, D, fallback ? 1 : 0);
    if (fallback) return;  // (per half wave; no barrier below)
    double* wt = W + ((size_t)w * 2 * KT + 2 * kt + hw) * APW_DCAP * NP * 32 + (size_t)wave * 32 + (lane & 31);  // + (d NL + l) NL 32: pair (l' = wave, l)
    // vw[q][e][lane] (LDS, this wave's own): the weights gathered so far for the four coefficients of the current interval (pair q = (l' = wave,
    // l = q)); when the walk moves to the next interval the window slides by one coefficient and the one that leaves is final.  In LDS rather
    // than in 24 registers, and the pairs in a rolled loop: the kernel has to fit beside two resummation waves on a SIMD (96 registers; with the
    // window in registers and the three pairs' gathers in flight together it needed 136)
    double* vw = sm + Nk + nmu + (size_t)wave * PPW * 4 * 64 + lane;
#pragma unroll
    for (int i = 0; i < PPW * 4; ++i) vw[i * 64] = 0.0;
    int Jc = 0, jb_prev = 0;
    for (int s = 0; s < (live ? nslot : 0); ++s) {
        const int i = i_first + s * dir;
        const double klo = s_k[i], khi = s_k[i + 1];
        const int ja = jb_prev;
        const int jb = s == nslot - 1 ? nmu : cross(up ? khi : klo);
        jb_prev = jb;
        const int Ji = bspl_first(i, Nk);
        if (s > 0 && Ji != Jc) {  // the window slides (by one: the walk visits neighbouring intervals): the coefficient that leaves is final
            const int dfin = (up ? Jc : Jc + 3) - jlow;
#pragma unroll
            for (int q = 0; q < PPW; ++q) {
                double* vq = vw + q * 4 * 64;
                const double v0 = vq[0], v1 = vq[64], v2 = vq[128], v3 = vq[192];
                wt[(size_t)(dfin * NL + q) * NL * 32] = up ? v0 : v3;
                vq[0] = up ? v1 : 0.0;
                vq[64] = up ? v2 : v0;
                vq[128] = up ? v3 : v1;
                vq[192] = up ? 0.0 : v2;
            }
        }
        Jc = Ji;
        if (jb > ja) {
            const double dl = kq - klo, dl2 = dl * dl, a2 = kq * kq;
            const char* psb = reinterpret_cast<const char*>(ps);  // wave-uniform base + 32-bit per-lane byte offsets (one address register, not two pointers)
            const unsigned oa = (unsigned)ja * NS * 8u, ob = (unsigned)jb * NS * 8u;
            const double4* lc = reinterpret_cast<const double4*>(LOCAL + (size_t)i * 16);
            // pair by pair: interval moments M_i[l'][l][p] of the nodes [ja, jb), then coefficient e of the interval takes sum_p M[p] local[i][e][p]
#pragma unroll 1
            for (int q = 0; q < PPW; ++q) {
                const unsigned p32 = (unsigned)(wave * NL + q) * 32u;  // the order of the prefix sums
                const double4 b4 = *reinterpret_cast<const double4*>(psb + (ob + p32)), a4 = *reinterpret_cast<const double4*>(psb + (oa + p32));
                const double d0 = b4.x - a4.x, d1 = b4.y - a4.y, d2 = b4.z - a4.z, d3 = b4.w - a4.w;
                const double m0 = d0, m1 = fma(dl, d0, kq * d1), m2 = fma(dl2, d0, fma(2.0 * kq * dl, d1, a2 * d2));
                const double m3 = fma(dl2 * dl, d0, fma(3.0 * kq * dl2, d1, fma(3.0 * a2 * dl, d2, a2 * kq * d3)));
                double* vq = vw + q * 4 * 64;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double4 n4 = lc[e];
                    vq[e * 64] = fma(m0, n4.x, fma(m1, n4.y, fma(m2, n4.z, fma(m3, n4.w, vq[e * 64]))));
                }
            }
        }
    }
    // the last interval's four coefficients, then zeros up to the tile's count (lanes past the grid: zeros throughout)
    if (live) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < PPW; ++q) wt[(size_t)((Jc + e - jlow) * NL + q) * NL * 32] = vw[(q * 4 + e) * 64];
    }
    for (int d = nD; d < D; ++d)
#pragma unroll
        for (int q = 0; q < PPW; ++q) wt[(size_t)(d * NL + q) * NL * 32] = 0.0;
}

// Workgroup = (tile of 32 k, cosmology) x NL waves; wave <-> output multipole l; lane = (k in the tile, half): half 0 owns the template
// rows [rlo, msplit), half 1 the rows [msplit, nr) (at most NH each).  LDS: the B-spline coefficients of every row in [rlo, nr) (rounded up to
// pairs) and every l' on the tile's window of APW_WIN knots -- [l'][row][knot], filled by global_load_lds (16 B per lane: one instruction = 64
// knots of two consecutive rows; no registers, every load of the workgroup in flight at once).  Every lane then walks the tile's D coefficients
// once, with the NL weights of the next RING - 1 coefficients in flight.  Rows outside [rlo, nr) are copied through from T.
// bias != null: the epilogue contracts P_l(k) = sum_row bias[row] out[l][row][k] as two FMA chains -- rows [0, msplit) in half 0, rows
// [msplit, NROW) in half 1 -- added across the half waves: the order of reduce_kernel(msplit), bit for bit.
template <int NL, int NH, int RING>
__global__ __launch_bounds__(64 * NL) void ap_rows_kernel(int Nk, int rlo, int nr, int msplit, const double* __restrict__ DAw, const double* __restrict__ Hw,
                                                          const double* __restrict__ fid, const double* __restrict__ W,
                                                          const int* __restrict__ I0, const int4* __restrict__ META,
                                                          const double* __restrict__ T, const double* __restrict__ C,
                                                          double* __restrict__ Tout, const double* __restrict__ bias, double* __restrict__ Plk,
                                                          double* __restrict__ PlkHost, int* __restrict__ nonfinite) {
    constexpr int NP = NL * NL;
    constexpr int nre = 2 * NH;  // window rows: [rlo, nr) rounded up to whole load instructions (host: nr - rlo <= nre, rlo + nre <= NROW)
    __shared__ double win[NL * nre * APW_WIN];
    const int lane = threadIdx.x & 63, l = threadIdx.x >> 6, kl = lane & 31, half = lane >> 5;
    const int KT = (Nk + 63) / 64, KT2 = 2 * KT;
    int kt, w;
    xcd_decode(KT2, kt, w);
    if (kt * 32 >= Nk) return;  // (the second half of the last 64-k tile may lie past the grid)
    const int4 meta = META[(size_t)w * KT2 + kt];
    if (meta.w) return;  // left to ap_direct_kernel
    const int k = kt * 32 + kl;
    const bool live = k < Nk;
    const int i0 = I0[(size_t)w * KT * 64 + k];
    const int jmin = meta.x, D = meta.z;
    {   // wave l stages l' = l: rows rlo .. rlo + nre - 1, coefficients jmin .. jmin + 63 (clamped to the row's end: those past the span carry no weight)
        // (a pair that starts at the last knot of a row ends one element past it -- the next row, or the two spare elements every template-
        // shaped buffer is allocated with; clamping to Nk - 2 instead would put coefficient Nk - 2 where coefficient Nk - 1 belongs)
        const double* src = C + (((size_t)w * NL + l) * NROW + rlo + half) * Nk + min(jmin + 2 * kl, Nk - 1);
        double* dst = win + (size_t)l * nre * APW_WIN;
#pragma unroll
        for (int r = 0; r < nre; r += 2)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)r * Nk),
                                             (__attribute__((address_space(3))) void*)(dst + r * APW_WIN), 16, 0, 0);
    }
    const double qperp = DAw[w] / fid[0], qpar = fid[1] / Hw[w];
    const double c = 2.0 / (qperp * qperp * qpar);
    const int q0 = half ? msplit : rlo, q1 = half ? nr : msplit, cnt = q1 - q0;  // this half's AP rows [q0, q1)
    const int o = max(i0 - jmin, 0);  // lanes past the grid (i0 = -1) carry zero weights
    const double* wt = W + ((size_t)w * KT2 + kt) * APW_DCAP * NP * 32 + (size_t)l * NL * 32 + kl;
    double acc[NH];
#pragma unroll
    for (int q = 0; q < NH; ++q) acc[q] = 0.0;
    // (branch-free: a ring slot past the tile's last coefficient holds zeros and re-reads the last one's rows -- with branches around the steps the
    // compiler speculates every LDS read of a step above its branch and the issue-order hints below no longer see them)
    double wr[RING][NL];
#pragma unroll
    for (int u = 0; u < RING; ++u) {
        const double* wn = wt + (size_t)min(u, D - 1) * NP * 32;
        const bool on = u < D;
#pragma unroll
        for (int lp = 0; lp < NL; ++lp) {
            const double a = wn[lp * 32];
            wr[u][lp] = on ? a : 0.0;
        }
    }
    __syncthreads();  // (drains the loads above: vmcnt(0) in front of the barrier)
    if (cnt > 0) {
        // row q of this half sits at window row q0 - rlo + q < nre (host: both halves hold at most NH rows): rows past the half's count read the
        // rows behind it (loaded, in bounds) and their sums are dropped -- every address below is one base register plus an immediate
        const double* yC = win + (size_t)(q0 - rlo) * APW_WIN + o;
        for (int d0 = 0; d0 < D; d0 += RING) {
#pragma unroll
            for (int u = 0; u < RING; ++u) {
                const int d = d0 + u;
#pragma unroll
                for (int lp = 0; lp < NL; ++lp)
#pragma unroll
                    for (int q = 0; q < NH; ++q) acc[q] = fma(wr[u][lp], yC[(lp * nre + q) * APW_WIN], acc[q]);
                yC += d + 1 < D ? 1 : 0;
                {   // this slot's next occupant: coefficient d + RING (zeros past the tile's last one)
                    const int dn = d + RING;
                    const double* wn = wt + (size_t)min(dn, D - 1) * NP * 32;
                    const bool on = dn < D;
#pragma unroll
                    for (int lp = 0; lp < NL; ++lp) {
                        const double a = wn[lp * 32];
                        wr[u][lp] = on ? a : 0.0;
                    }
                }
                // issue order of this step's NL * NH LDS reads (one or two rows each) and FMAs: APR_AHEAD reads ahead, then one read per two
                // FMAs -- left alone the scheduler puts every read of the step in front of the first FMA
                constexpr int AHEAD = APR_AHEAD;
                __builtin_amdgcn_sched_group_barrier(0x100, AHEAD, 0);
#pragma unroll
                for (int i = 0; i < (NL * NH) / 2 - AHEAD; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x002, 2 * AHEAD + 16, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // results, the rows APeffect leaves alone (Pstl unless APst; everything but the counter-term rows of the NNLO block), and the contraction
    const size_t obase = (((size_t)w * NL + l) * NROW) * Nk + k;
    const double* bw = bias ? bias + (size_t)w * NROW : nullptr;
    double a = 0.0;
    if (live) {
        const int hlo = half ? msplit : 0, hhi = half ? NROW : msplit;  // this half's share of the NROW rows in the contraction
        for (int r = hlo; r < min(q0, hhi); ++r) {
            const double v = T[obase + (size_t)r * Nk];
            Tout[obase + (size_t)r * Nk] = v;
            if (bw) a = fma(bw[r], v, a);
        }
#pragma unroll
        for (int q = 0; q < NH; ++q)
            if (q < cnt) {
                const double v = c * acc[q];
                Tout[obase + (size_t)(q0 + q) * Nk] = v;
                if (bw) a = fma(bw[q0 + q], v, a);
            }
        for (int r = max(q1, hlo); r < hhi; ++r) {
            const double v = T[obase + (size_t)r * Nk];
            Tout[obase + (size_t)r * Nk] = v;
            if (bw) a = fma(bw[r], v, a);
        }
    }
    if (bias) {
        const double other = __shfl_xor(a, 32);
        const double tot = half ? other + a : a + other;  // rows [0, msplit) + rows [msplit, NROW)
        if (live && half == 0) {
            Plk[((size_t)w * NL + l) * Nk + k] = tot;
            if (PlkHost) PlkHost[((size_t)w * NL + l) * Nk + k] = tot;  // latency mode: P_l lands in mapped host memory as it is formed
            if (nonfinite && !(fabs(tot) <= 1.79769313486231570815e308)) atomicMax(nonfinite, w + 1);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// AP of direct-P_l runs (EFTB_O_PLK_DIRECT): ONE row per multipole goes through the stage, and for one row the reference's own form
// (pybird.py:1581-1621: the nmu-node quadrature of P_l'(k'(mu)) L_l'(mu') L_l(mu), row 0 of the block already contracted with the bias) is
// cheaper than the knot-weight tables, which pay off over the 21 rows of a template block: no prefix sums, no weights, no banded product.
// Workgroup = (64 k, cosmology) x 4 waves; wave <-> a quarter of the nodes, lane <-> k.  LDS: per node {root, L_2(mu'), L_4(mu'), w L_l(mu)}
// (the cosmology's, built once per workgroup), and the spline of the three l' in piecewise-polynomial form on the window of knot intervals
// the tile's k'(mu) can reach (from the B-spline coefficients of spline_kernel and the per-interval matrices, tables.bspline_tables): a
// node then costs three cubics, three Legendre weights and three accumulations per lane.  Windows wider than APD_WMAX intervals (distortions
// beyond ~20 % at the top of the grid) take the same walk with the pieces formed from global memory.  The four partial sums meet in LDS in
// wave order; the epilogue adds the rows outside the stage (from direct0 on: the stochastic templates) times their bias coefficients.
// ------------------------------------------------------------------------------------------------
constexpr int APD_WMAX = 192;

template <int NL>
__global__ __launch_bounds__(256) void ap_plk_kernel(int Nk, int nmu, const double* __restrict__ kk, const double* __restrict__ DAw,
                                                     const double* __restrict__ Hw, const double* __restrict__ fid, const double* __restrict__ mu,
                                                     const double* __restrict__ wmu, const double* __restrict__ legmu, const double* __restrict__ C,
                                                     const double* __restrict__ LOCAL, const double* __restrict__ T, const double* __restrict__ bias,
                                                     double* __restrict__ Plk, double* __restrict__ PlkHost, int* __restrict__ nonfinite, int direct0) {
    extern __shared__ double sm[];
    double* s_k = sm;                           // [Nk] (+ 1 if odd) the k grid (every interval search below is an LDS walk)
    double* s_node = s_k + ((Nk + 1) & ~1);     // [nmu][8]  (16-byte aligned for an odd Nk too: read and written 32 bytes at a time, like s_pp behind it)
    double* s_pp = s_node + (size_t)nmu * 8;    // [NL][APD_WMAX][4]
    double* s_red = s_pp + NL * APD_WMAX * 4;   // [3][NL][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int KT = (Nk + 63) / 64;
    int kt, w;
    xcd_decode(KT, kt, w);
    const int k = kt * 64 + lane, kc = min(k, Nk - 1);
    const double qperp = DAw[w] / fid[0], qpar = fid[1] / Hw[w];
    const double F = qpar / qperp, g = 1.0 / (F * F) - 1.0, cnorm = 2.0 / (qperp * qperp * qpar);
    for (int e = threadIdx.x; e < Nk; e += blockDim.x) s_k[e] = kk[e];
    for (int j = threadIdx.x; j < nmu; j += blockDim.x) {
        const double m = mu[j], root = sqrt(1.0 + m * m * g), mp = m / (F * root), x2 = mp * mp, wj = wmu[j];
        double* nd = s_node + (size_t)j * 8;
        nd[0] = root;
        nd[1] = 0.5 * (3.0 * x2 - 1.0);
        nd[2] = (35.0 * x2 * x2 - 30.0 * x2 + 3.0) * 0.125;
        nd[3] = 0.0;
#pragma unroll
        for (int l = 0; l < NL; ++l) nd[4 + l] = wj * legmu[(size_t)l * nmu + j];
    }
    __syncthreads();
    // the window: every interval a k of this tile can reach (k'(mu) = k / q_perp root(mu), root monotonic in mu)
    const double r0 = s_node[0], r1 = s_node[(size_t)(nmu - 1) * 8];
    const double ka = s_k[kt * 64] / qperp, kb = s_k[min(kt * 64 + 63, Nk - 1)] / qperp;
    const int wlo = knot_interval(s_k, Nk, ka * fmin(r0, r1)), whi = knot_interval(s_k, Nk, kb * fmax(r0, r1)), nwin = whi - wlo + 1;
    const bool big = nwin > APD_WMAX;  // (workgroup-uniform)
    const double* cw = C + (size_t)w * NL * NROW * Nk;  // row 0 of every l' block
    if (!big) {
        for (int e = threadIdx.x; e < nwin * NL; e += blockDim.x) {
            const int iw = e % nwin, lp = e / nwin, i = wlo + iw, J = bspl_first(i, Nk);
            const double* cp = cw + (size_t)lp * NROW * Nk + J;
            const double c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3];
            const double4* lc = reinterpret_cast<const double4*>(LOCAL + (size_t)i * 16);
            const double4 e0 = lc[0], e1 = lc[1], e2 = lc[2], e3 = lc[3];
            double4 pp;
            pp.x = fma(e0.x, c0, fma(e1.x, c1, fma(e2.x, c2, e3.x * c3)));
            pp.y = fma(e0.y, c0, fma(e1.y, c1, fma(e2.y, c2, e3.y * c3)));
            pp.z = fma(e0.z, c0, fma(e1.z, c1, fma(e2.z, c2, e3.z * c3)));
            pp.w = fma(e0.w, c0, fma(e1.w, c1, fma(e2.w, c2, e3.w * c3)));
            *reinterpret_cast<double4*>(s_pp + ((size_t)lp * APD_WMAX + iw) * 4) = pp;
        }
    }
    __syncthreads();
    const int nq = (nmu + 3) / 4, j0 = wave * nq, j1 = min(nmu, j0 + nq);
    const double kq = s_k[kc] / qperp;
    double acc[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) acc[l] = 0.0;
    // the pieces of the interval the lane stands in live in registers and are replaced only when k'(mu) leaves it; the walk is compiled twice
    // (window in LDS / pieces from global memory: workgroup-uniform choice) so that the common form carries none of the other's code
    auto walk = [&](auto bigc) {
        constexpr bool BIG = decltype(bigc)::value;
        auto piece = [&](int i, double4 (&a)[NL]) {
            if constexpr (!BIG) {
#pragma unroll
                for (int lp = 0; lp < NL; ++lp) a[lp] = *reinterpret_cast<const double4*>(s_pp + ((size_t)lp * APD_WMAX + (i - wlo)) * 4);
            } else {
                const double4* lc = reinterpret_cast<const double4*>(LOCAL + (size_t)i * 16);
                const double4 e0 = lc[0], e1 = lc[1], e2 = lc[2], e3 = lc[3];
                const int J = bspl_first(i, Nk);
#pragma unroll
                for (int lp = 0; lp < NL; ++lp) {
                    const double* cp = cw + (size_t)lp * NROW * Nk + J;
                    const double c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3];
                    a[lp].x = fma(e0.x, c0, fma(e1.x, c1, fma(e2.x, c2, e3.x * c3)));
                    a[lp].y = fma(e0.y, c0, fma(e1.y, c1, fma(e2.y, c2, e3.y * c3)));
                    a[lp].z = fma(e0.z, c0, fma(e1.z, c1, fma(e2.z, c2, e3.z * c3)));
                    a[lp].w = fma(e0.w, c0, fma(e1.w, c1, fma(e2.w, c2, e3.w * c3)));
                }
            }
        };
        int i = knot_interval(s_k, Nk, kq * s_node[(size_t)j0 * 8]);
        double klo = s_k[i], khi = s_k[i + 1];
        double4 a[NL];
        piece(i, a);
        for (int j = j0; j < j1; ++j) {
            const double4 n0 = *reinterpret_cast<const double4*>(s_node + (size_t)j * 8), n1 = *reinterpret_cast<const double4*>(s_node + (size_t)j * 8 + 4);
            const double kp = kq * n0.x;
            // interval changes as WAVE-uniform steps: some lane of the wave crosses a knot at almost every node, so a per-lane branch is taken
            // (by everybody) nearly always -- one step of every lane that has to move, the loop repeats only while some lane is still outside
            // its interval (the end intervals extrapolate: the reference's comparison k_i <= k' < k_i+1), then one reload of the pieces
            bool moved = false;
            for (;;) {
                const bool up = kp >= khi && i < Nk - 2, dn = kp < klo && i > 0;
                if (!__any(up || dn)) break;
                i += (up ? 1 : 0) - (dn ? 1 : 0);
                klo = s_k[i];
                khi = s_k[i + 1];
                moved = true;
            }
            if (moved) piece(i, a);  // (wave-uniform)
            const double t = kp - klo;
            double P = fma(fma(fma(a[0].w, t, a[0].z), t, a[0].y), t, a[0].x);
            P = fma(fma(fma(fma(a[1].w, t, a[1].z), t, a[1].y), t, a[1].x), n0.y, P);
            if (NL > 2) P = fma(fma(fma(fma(a[NL - 1].w, t, a[NL - 1].z), t, a[NL - 1].y), t, a[NL - 1].x), n0.z, P);
            acc[0] = fma(n1.x, P, acc[0]);
            acc[1] = fma(n1.y, P, acc[1]);
            if (NL > 2) acc[NL - 1] = fma(n1.z, P, acc[NL - 1]);
        }
    };
    if (j0 < j1) {
        if (big) walk(std::true_type{});
        else walk(std::false_type{});
    }
    if (wave > 0) {
#pragma unroll
        for (int l = 0; l < NL; ++l) s_red[((size_t)(wave - 1) * NL + l) * 64 + lane] = acc[l];
    }
    __syncthreads();
    if (wave > 0 || k >= Nk) return;
    const double* bw = bias + (size_t)w * NROW;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        double a = acc[l];
#pragma unroll
        for (int q = 0; q < 3; ++q) a += s_red[((size_t)q * NL + l) * 64 + lane];
        double tot = cnorm * a;
        for (int r = direct0; r < NROW; ++r) tot = fma(bw[r], stoch_template(l, r - (NROW - 3), kk[k]), tot);   // (direct0 = NROW - 3 or NROW)
        Plk[((size_t)w * NL + l) * Nk + k] = tot;
        if (PlkHost) PlkHost[((size_t)w * NL + l) * Nk + k] = tot;  // latency mode: P_l lands in mapped host memory as it is formed
        if (nonfinite && !(fabs(tot) <= 1.79769313486231570815e308)) atomicMax(nonfinite, w + 1);
    }
}

// ------------------------------------------------------------------------------------------------
// AP of direct-P_l runs, moment form (round 4; ap_plk_kernel above is kept for A/B runs, EFTB_AP_PLK_NODES=1).  The node quadrature of one
// contracted row costs ~50 instructions per (k, node) in dependent LDS chains and fills every SIMD with waiting waves for 40-60 us.  But P_l' is a
// piecewise cubic, so the nmu-node sum over the nodes that fall into knot interval i is a combination of four interval moments,
//     sum_{j in [ja, jb)} wl[l][j] lp[l'][j] P_l'(k'_j) = sum_p a_i[l'][p] M_i[l][l'][p],
// and the moments are binomial combinations of the k-independent mu prefix sums of ap_prefix_kernel (header above it): per (k, interval
// crossed) 36 prefix differences, 90 FMAs for the binomials, 36 for the contraction -- no node loop.  A k crosses 1 ... ~10 intervals at the
// distortions a chain visits (cost grows with the distortion; any number is handled).  Same sum as the reference's quadrature
// (pybird.py:1581-1621) in another order.
// Workgroup = (64 k, cosmology) x 4 waves; wave <-> interval slot (s = wave, wave + 4, ...) exactly as in ap_moments_kernel; the pieces of
// interval i come from the B-spline coefficients of spline_kernel (row 0 of each l' block) and the per-interval matrices
// (tables.bspline_tables); the four partial sums meet in LDS in wave order; the epilogue adds the rows outside the stage (from direct0 on:
// the stochastic templates) times their bias coefficients.
// ------------------------------------------------------------------------------------------------
template <int NL>
__global__ __launch_bounds__(256) void ap_plk_mom_kernel(int Nk, int nmu, const double* __restrict__ kk, const double* __restrict__ DAw,
                                                         const double* __restrict__ Hw, const double* __restrict__ fid, const double* __restrict__ mu,
                                                         const double* __restrict__ PS, const double* __restrict__ ROOT, const double* __restrict__ C,
                                                         const double* __restrict__ LOCAL, const double* __restrict__ T, const double* __restrict__ bias,
                                                         double* __restrict__ Plk, double* __restrict__ PlkHost, int* __restrict__ nonfinite, int direct0) {
    constexpr int NSQ = NL * NL * 4;
    extern __shared__ double sm[];
    double* s_k = sm;               // [Nk]
    double* s_root = sm + Nk;       // [nmu]
    double* red = sm + Nk + nmu;    // [3][NL][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int KT = (Nk + 63) / 64;
    int kt, w;
    xcd_decode(KT, kt, w);
    const int k = kt * 64 + lane;
    for (int e = threadIdx.x; e < Nk; e += 256) s_k[e] = kk[e];
    for (int e = threadIdx.x; e < nmu; e += 256) s_root[e] = ROOT[(size_t)w * nmu + e];
    __syncthreads();
    const double qperp = DAw[w] / fid[0], qpar = fid[1] / Hw[w];
    const double F = qpar / qperp, g = 1.0 / (F * F) - 1.0;
    const bool live = k < Nk;
    const double kq = s_k[live ? k : Nk - 1] / qperp;
    const double inv_kq = 1.0 / kq, inv_g = 1.0 / g;
    const double* ps = PS + (size_t)w * (nmu + 1) * NSQ;
    const double* cw = C + (size_t)w * NL * NROW * Nk;  // row 0 of every l' block
    const bool up = g > 0.0;  // k'(mu) rises or falls with mu
    const int dir = up ? 1 : -1;
    const double jscale = (nmu - 1) / mu[nmu - 1];  // node index per unit mu (uniform grid: only a first guess, see the fix-up)
    double acc[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) acc[l] = 0.0;
    // first node that lies past knot kb (k'_j >= kb when rising, k'_j < kb when falling)
    auto cross = [&](double kb) -> int {
        const double rc = kb * inv_kq, x = (rc * rc - 1.0) * inv_g;  // mu^2 at the crossing (a seed: the fix-up below decides)
        int j = nmu;
        if (x >= 0.0 && x < 1.0) j = (int)(sqrt(x) * jscale) + 1;
        j = max(0, min(j, nmu));
        while (j > 0 && (up ? kq * s_root[j - 1] >= kb : kq * s_root[j - 1] < kb)) --j;
        while (j < nmu && !(up ? kq * s_root[j] >= kb : kq * s_root[j] < kb)) ++j;
        return j;
    };
    const int i_first = knot_interval(s_k, Nk, kq * s_root[0]);
    const int i_last = knot_interval(s_k, Nk, kq * s_root[nmu - 1]);
    const int nslot = live ? (up ? i_last - i_first : i_first - i_last) + 1 : 0;
    for (int s = wave; s < nslot; s += 4) {
        const int i = i_first + s * dir;
        const double klo = s_k[i], khi = s_k[i + 1];
        const int ja = s == 0 ? 0 : cross(up ? klo : khi);
        const int jb = s == nslot - 1 ? nmu : cross(up ? khi : klo);
        if (jb <= ja) continue;
        // everything this slot reads is requested before anything is used: prefix sums at both ends, the interval's matrices, the coefficients
        const double* pa = ps + (size_t)ja * NSQ;
        const double* pb = ps + (size_t)jb * NSQ;
        double4 a4[NL][NL], b4[NL][NL];
#pragma unroll
        for (int lp = 0; lp < NL; ++lp)
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                b4[lp][l] = *reinterpret_cast<const double4*>(pb + (lp * NL + l) * 4);
                a4[lp][l] = *reinterpret_cast<const double4*>(pa + (lp * NL + l) * 4);
            }
        const double4* lc = reinterpret_cast<const double4*>(LOCAL + (size_t)i * 16);
        const double4 e0 = lc[0], e1 = lc[1], e2 = lc[2], e3 = lc[3];
        const int J = bspl_first(i, Nk);
        double cc[NL][4];
#pragma unroll
        for (int lp = 0; lp < NL; ++lp) {
            const double* cp = cw + (size_t)lp * NROW * Nk + J;
            cc[lp][0] = cp[0]; cc[lp][1] = cp[1]; cc[lp][2] = cp[2]; cc[lp][3] = cp[3];
        }
        const double dl = kq - klo, dl2 = dl * dl, a2 = kq * kq;
        const double c10 = dl, c11 = kq, c20 = dl2, c21 = 2.0 * kq * dl, c22 = a2;
        const double c30 = dl2 * dl, c31 = 3.0 * kq * dl2, c32 = 3.0 * a2 * dl, c33 = a2 * kq;
#pragma unroll
        for (int lp = 0; lp < NL; ++lp) {
            // power form of P_l' on [k_i, k_i+1] in t = k' - k_i
            const double p0 = fma(e0.x, cc[lp][0], fma(e1.x, cc[lp][1], fma(e2.x, cc[lp][2], e3.x * cc[lp][3])));
            const double p1 = fma(e0.y, cc[lp][0], fma(e1.y, cc[lp][1], fma(e2.y, cc[lp][2], e3.y * cc[lp][3])));
            const double p2 = fma(e0.z, cc[lp][0], fma(e1.z, cc[lp][1], fma(e2.z, cc[lp][2], e3.z * cc[lp][3])));
            const double p3 = fma(e0.w, cc[lp][0], fma(e1.w, cc[lp][1], fma(e2.w, cc[lp][2], e3.w * cc[lp][3])));
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double d0 = b4[lp][l].x - a4[lp][l].x, d1 = b4[lp][l].y - a4[lp][l].y;
                const double d2 = b4[lp][l].z - a4[lp][l].z, d3 = b4[lp][l].w - a4[lp][l].w;
                const double m1 = fma(c10, d0, c11 * d1);
                const double m2 = fma(c20, d0, fma(c21, d1, c22 * d2));
                const double m3 = fma(c30, d0, fma(c31, d1, fma(c32, d2, c33 * d3)));
                acc[l] = fma(d0, p0, fma(m1, p1, fma(m2, p2, fma(m3, p3, acc[l]))));
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int l = 0; l < NL; ++l) red[((size_t)(wave - 1) * NL + l) * 64 + lane] = acc[l];
    }
    __syncthreads();
    if (wave > 0 || !live) return;
    const double cnorm = 2.0 / (qperp * qperp * qpar);
    const double* bw = bias + (size_t)w * NROW;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        double a = acc[l];
#pragma unroll
        for (int q = 0; q < 3; ++q) a += red[((size_t)q * NL + l) * 64 + lane];
        double tot = cnorm * a;
        for (int r = direct0; r < NROW; ++r) tot = fma(bw[r], stoch_template(l, r - (NROW - 3), kk[k]), tot);   // (direct0 = NROW - 3 or NROW)
        Plk[((size_t)w * NL + l) * Nk + k] = tot;
        if (PlkHost) PlkHost[((size_t)w * NL + l) * Nk + k] = tot;  // latency mode: P_l lands in mapped host memory as it is formed
        if (nonfinite && !(fabs(tot) <= 1.79769313486231570815e308)) atomicMax(nonfinite, w + 1);
    }
}

// ------------------------------------------------------------------------------------------------
// ap_plk_fused_kernel: the whole AP stage of a direct-P_l run behind the spline coefficients in ONE launch, one workgroup per (cosmology, half of
// the k tiles), everything it gathers from in LDS:
//   1. the mu tables of the cosmology (rho_j, L_l'(mu'_j), w_j L_l(mu_j)) and their prefix sums PS[j][l'][l][q] (what ap_prefix_kernel writes to
//      global memory: 58 KB that every (k, interval) of ap_plk_mom_kernel gathers 2 x 288 bytes from, one HBM / L2 round trip per interval),
//   2. the power-form pieces of the three contracted splines on every knot interval (B-spline coefficients x per-interval matrices: 48 KB),
//   3. per k the walk over the intervals k'(mu) crosses, moments by differences of the prefix sums (header of ap_plk_mom_kernel), all reads LDS.
// One workgroup of eight waves per cosmology (NW = 8; or two of four, NW = 4): 23 us alone at B = 128 for spline-to-P_l against 35 (4 096 waves of
// 156 registers gathering from global memory + ap_prefix_kernel) -- beside it the rest of the machine stays free for the other streams' kernels.  Needs (nmu + 1) 36 + Nk 12 + ... doubles
// of LDS: k grids up to 768 points; finer grids keep ap_prefix_kernel + ap_plk_mom_kernel.
// ------------------------------------------------------------------------------------------------
template <int NL, int NW>
__global__ __launch_bounds__(64 * NW) void ap_plk_fused_kernel(int Nk, int nmu, const double* __restrict__ kk, const double* __restrict__ DAw,
                                                           const double* __restrict__ Hw, const double* __restrict__ fid, const double* __restrict__ mu,
                                                           const double* __restrict__ wmu, const double* __restrict__ legmu, const double* __restrict__ C,
                                                           const double* __restrict__ LOCAL, const double* __restrict__ T, const double* __restrict__ bias,
                                                           double* __restrict__ Plk, double* __restrict__ PlkHost, int* __restrict__ nonfinite, int direct0) {
    constexpr int NSQ = NL * NL * 4, NT = 64 * NW, NCHK = NT / NSQ;   // 36 sequences x 7 (14) chunks of the mu range = 252 (504) threads
    extern __shared__ double sm[];
    double* s_k = sm;                                   // [Nk] (+ 1 if odd)
    double* s_root = s_k + ((Nk + 1) & ~1);             // [nmu]
    double* s_rho = s_root + nmu;                       // [nmu]
    double* s_lp = s_rho + nmu;                         // [NL][nmu]  L_l'(mu')
    double* s_wl = s_lp + NL * nmu;                     // [NL][nmu]  wmu (2l+1)/2 L_l(mu)
    double* s_tot = s_wl + NL * nmu;                    // [NSQ][NCHK + 1]
    double* s_ps = s_tot + NSQ * (NCHK + 1);            // [nmu + 1][NSQ]
    double* s_pp = s_ps + (size_t)(nmu + 1) * NSQ;      // [Nk - 1][NL][4]  (16-byte aligned: every block above has an even length)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int SPLIT = NW == 8 ? 1 : 2;   // workgroups per cosmology: eight waves take every tile of a cosmology, four waves every other one
    const int half = blockIdx.x % SPLIT, w = blockIdx.x / SPLIT;
    const double qperp = DAw[w] / fid[0], qpar = fid[1] / Hw[w];
    const double F = qpar / qperp, g = 1.0 / (F * F) - 1.0;
    // ---- 1. tables
    for (int e = threadIdx.x; e < Nk; e += NT) s_k[e] = kk[e];
    for (int j = threadIdx.x; j < nmu; j += NT) {
        const double m = mu[j];
        const double root = sqrt(1.0 + m * m * g);
        const double mp = m / (F * root), x2 = mp * mp, wj = wmu[j];
        s_root[j] = root;
        s_rho[j] = g * m * m / (1.0 + root);
        s_lp[j] = 1.0;
        s_lp[nmu + j] = 0.5 * (3.0 * x2 - 1.0);
        if (NL > 2) s_lp[2 * nmu + j] = (35.0 * x2 * x2 - 30.0 * x2 + 3.0) * 0.125;
#pragma unroll
        for (int l = 0; l < NL; ++l) s_wl[l * nmu + j] = wj * legmu[(size_t)l * nmu + j];
    }
    // ---- 2. pieces: interval i of spline l' in power form (t = k' - k_i)
    const double* cw = C + (size_t)w * NL * NROW * Nk;  // row 0 of every l' block
    for (int i = threadIdx.x; i < Nk - 1; i += NT) {
        const int J = bspl_first(i, Nk);
        const double4* lc = reinterpret_cast<const double4*>(LOCAL + (size_t)i * 16);
        const double4 e0 = lc[0], e1 = lc[1], e2 = lc[2], e3 = lc[3];
        double cc[NL][4];
#pragma unroll
        for (int lp = 0; lp < NL; ++lp) {
            const double* cp = cw + (size_t)lp * NROW * Nk + J;
            cc[lp][0] = cp[0]; cc[lp][1] = cp[1]; cc[lp][2] = cp[2]; cc[lp][3] = cp[3];
        }
#pragma unroll
        for (int lp = 0; lp < NL; ++lp) {
            const double c0 = cc[lp][0], c1 = cc[lp][1], c2 = cc[lp][2], c3 = cc[lp][3];
            double4 pp;
            pp.x = fma(e0.x, c0, fma(e1.x, c1, fma(e2.x, c2, e3.x * c3)));
            pp.y = fma(e0.y, c0, fma(e1.y, c1, fma(e2.y, c2, e3.y * c3)));
            pp.z = fma(e0.z, c0, fma(e1.z, c1, fma(e2.z, c2, e3.z * c3)));
            pp.w = fma(e0.w, c0, fma(e1.w, c1, fma(e2.w, c2, e3.w * c3)));
            *reinterpret_cast<double4*>(s_pp + ((size_t)i * NL + lp) * 4) = pp;
        }
    }
    __syncthreads();
    // ---- prefix sums over mu, PS[j][l'][l][q] = sum_{j' < j} wl[l][j'] lp[l'][j'] rho_j'^q: thread <-> (sequence, chunk of <= 32 nodes).  The chunk's
    // terms are formed in registers (independent LDS reads, all in flight at once), summed there, and written once behind the chunk offsets --
    // ap_prefix_kernel's two sweeps with their LDS round trip per node were 6 us of this kernel's 25
    {
        constexpr int CL = NW == 8 ? 16 : 32;
        const int seq = threadIdx.x % NSQ, ch = threadIdx.x / NSQ;
        const int q = seq & 3, l = (seq >> 2) % NL, lp = seq / (4 * NL);
        const int clen = (nmu + NCHK - 1) / NCHK, j0 = ch * clen, nj = ch < NCHK ? max(0, min(nmu - j0, clen)) : 0;  // (host: clen <= CL)
        double v[CL];
#pragma unroll
        for (int u = 0; u < CL; ++u) {
            const int j = min(j0 + u, nmu - 1);
            const double r = s_rho[j];
            const double rq = q == 0 ? 1.0 : (q == 1 ? r : (q == 2 ? r * r : r * r * r));
            v[u] = u < nj ? s_wl[l * nmu + j] * s_lp[lp * nmu + j] * rq : 0.0;
        }
#pragma unroll
        for (int u = 1; u < CL; ++u) v[u] += v[u - 1];
        if (ch < NCHK) s_tot[seq * (NCHK + 1) + ch] = v[CL - 1];
        __syncthreads();
        if (threadIdx.x < NSQ) {  // exclusive scan of the chunk totals
            double run = 0.0;
            for (int c = 0; c < NCHK; ++c) {
                const double t = s_tot[threadIdx.x * (NCHK + 1) + c];
                s_tot[threadIdx.x * (NCHK + 1) + c] = run;
                run += t;
            }
            s_ps[threadIdx.x] = 0.0;
        }
        __syncthreads();
        if (ch < NCHK) {
            const double off = s_tot[seq * (NCHK + 1) + ch];
#pragma unroll
            for (int u = 0; u < CL; ++u)
                if (u < nj) s_ps[(size_t)(j0 + u + 1) * NSQ + seq] = off + v[u];
        }
    }
    __syncthreads();
    // ---- 3. the k tiles of this half, one per wave at a time (tiles interleave between the two halves: the high-k tiles cross more intervals)
    const int KT = (Nk + 63) / 64;
    const bool up = g > 0.0;  // k'(mu) rises or falls with mu
    const int dir = up ? 1 : -1;
    const double inv_g = 1.0 / g, jscale = (nmu - 1) / mu[nmu - 1];
    const double cnorm = 2.0 / (qperp * qperp * qpar);
    const double* bw = bias + (size_t)w * NROW;
    for (int kt = SPLIT * wave + half; kt < KT; kt += SPLIT * NW) {
        const int k = kt * 64 + lane;
        const bool live = k < Nk;
        const double kq = s_k[live ? k : Nk - 1] / qperp, inv_kq = 1.0 / kq;
        // (the rows outside the stage: requested now, consumed behind the walk)
        double tst[NL][3];
#pragma unroll
        for (int l = 0; l < NL; ++l)
#pragma unroll
            for (int r = 0; r < 3; ++r) tst[l][r] = live && NROW - 3 + r >= direct0 ? stoch_template(l, r, s_k[k]) : 0.0;
        auto cross = [&](double kb) -> int {  // first node that lies past knot kb (k'_j >= kb when rising, k'_j < kb when falling)
            const double rc = kb * inv_kq, x = (rc * rc - 1.0) * inv_g;  // mu^2 at the crossing (a seed: the fix-up below decides)
            int j = nmu;
            if (x >= 0.0 && x < 1.0) j = (int)(sqrt(x) * jscale) + 1;
            j = max(0, min(j, nmu));
            while (j > 0 && (up ? kq * s_root[j - 1] >= kb : kq * s_root[j - 1] < kb)) --j;
            while (j < nmu && !(up ? kq * s_root[j] >= kb : kq * s_root[j] < kb)) ++j;
            return j;
        };
        const int i_first = knot_interval(s_k, Nk, kq * s_root[0]);
        const int i_last = knot_interval(s_k, Nk, kq * s_root[nmu - 1]);
        const int nslot = live ? (up ? i_last - i_first : i_first - i_last) + 1 : 0;
        double acc[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) acc[l] = 0.0;
        int ja = 0;
        for (int s = 0; s < nslot; ++s) {
            const int i = i_first + s * dir;
            const double klo = s_k[i], khi = s_k[i + 1];
            const int jb = s == nslot - 1 ? nmu : cross(up ? khi : klo);
            if (jb > ja) {
                // P_l'(k') on this interval as a cubic in rho (k' - k_i = kq rho + dl): sum_j W_j P(k'_j) = sum_q w_q (PS_q[jb] - PS_q[ja])
                const double dl = kq - klo, kq2 = kq * kq;
                const double* pa = s_ps + (size_t)ja * NSQ;
                const double* pb = s_ps + (size_t)jb * NSQ;
                const double* pi = s_pp + (size_t)i * NL * 4;
#pragma unroll
                for (int lp = 0; lp < NL; ++lp) {
                    const double4 p = *reinterpret_cast<const double4*>(pi + lp * 4);
                    const double w0 = fma(fma(fma(p.w, dl, p.z), dl, p.y), dl, p.x);
                    const double w1 = kq * fma(fma(3.0 * p.w, dl, 2.0 * p.z), dl, p.y);
                    const double w2 = kq2 * fma(3.0 * p.w, dl, p.z);
                    const double w3 = kq2 * kq * p.w;
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        const double4 b4 = *reinterpret_cast<const double4*>(pb + (lp * NL + l) * 4);
                        const double4 a4 = *reinterpret_cast<const double4*>(pa + (lp * NL + l) * 4);
                        acc[l] = fma(b4.x - a4.x, w0, fma(b4.y - a4.y, w1, fma(b4.z - a4.z, w2, fma(b4.w - a4.w, w3, acc[l]))));
                    }
                }
                ja = jb;
            }
        }
        if (!live) continue;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            double tot = cnorm * acc[l];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (NROW - 3 + r >= direct0) tot = fma(bw[NROW - 3 + r], tst[l][r], tot);
            Plk[((size_t)w * NL + l) * Nk + k] = tot;
            if (PlkHost) PlkHost[((size_t)w * NL + l) * Nk + k] = tot;  // latency mode: P_l lands in mapped host memory as it is formed
            if (nonfinite && !(fabs(tot) <= 1.79769313486231570815e308)) atomicMax(nonfinite, w + 1);
        }
    }
}

// Staged inputs: page-locked host block -> device block, as a kernel on the copy stream (a DMA transfer brings cache maintenance on the
// compute queue with it; this one is ordinary loads from mapped host memory and ordinary stores)
__global__ __launch_bounds__(256) void stage_copy_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// The same for a launch that carries several queued steps: up to 8 steps x 6 arrays, each a run of doubles from a step's staging block to its rows
// of the device block.  One double per lane and every load of the launch in flight at once: the reads cross PCIe (1.5-2 us each way), so the
// kernel's time is one round trip + the transfer, not a chain of them (12 workgroups per run walking it in 8 passes took 45-56 us for 0.23 MB).
struct StageSeg { const double* src; double* dst; unsigned n, first; };   // first: index of the run's first element in the launch's flat numbering (multiples of 64)
struct StageSegs { StageSeg s[48]; int n; };
__global__ __launch_bounds__(256) void stage_gather_kernel(StageSegs sg) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    int seg = 0;
    for (int q = 1; q < sg.n; ++q)
        if (i >= sg.s[q].first) seg = q;   // (runs start at multiples of 64: the choice is wave-uniform)
    const StageSeg g = sg.s[seg];
    const unsigned j = i - g.first;
    if (j < g.n) g.dst[j] = g.src[j];
}

// nothing: the first dispatch after the GPU has sat idle for a few tens of microseconds takes 40-50 us to start executing (traced: a 27 KB copy
// kernel 44 us, the 205 KB one behind it 6 us) -- eftb_stage_inputs sends this ahead of its host-side work so that the step's first real kernel
// finds the queue awake
__global__ void wake_kernel() {}

// P_l of a pipelined step -> mapped page-locked host memory, 16 bytes per lane, a few dozen workgroups: the PCIe stores keep 48 waves busy
// instead of the 4 096 of the kernel that forms P_l
__global__ __launch_bounds__(256) void copy16_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
    const size_t n2 = n / 2;
    const double2* s2 = reinterpret_cast<const double2*>(src);
    double2* d2 = reinterpret_cast<double2*>(dst);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) d2[i] = s2[i];
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = src[n - 1];
}

// the same with 8 bytes per lane: for a source or destination that is only 8-byte aligned (an odd row length and a step that starts at an odd row)
__global__ __launch_bounds__(256) void copy8_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------
// reduce: P_l(k) = sum_row bias[row] * T[l][row][k]  (reference parambasis.py:128-136)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reduce_kernel(int Nx, int Nl, int msplit, const double* __restrict__ bias, const double* __restrict__ T,
                                                     double* __restrict__ Plk, double* __restrict__ PlkHost, int* __restrict__ nonfinite) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y, w = blockIdx.z;
    if (k >= Nx) return;
    const double* b = bias + (size_t)w * NROW;
    const double* t = T + (((size_t)w * Nl + l) * NROW) * Nx + k;
    // two FMA chains, rows [0, msplit) and [msplit, NROW), then their sum: the order in which ap_rows_kernel's two half waves contract when
    // REDUCE follows the AP stage directly -- a stand-alone REDUCE gives the same bits
    double a0 = 0.0, a1 = 0.0;
    for (int r = 0; r < msplit; ++r) a0 = fma(b[r], t[(size_t)r * Nx], a0);
    for (int r = msplit; r < NROW; ++r) a1 = fma(b[r], t[(size_t)r * Nx], a1);
    const double a = a0 + a1;
    Plk[((size_t)w * Nl + l) * Nx + k] = a;
    if (PlkHost) PlkHost[((size_t)w * Nl + l) * Nx + k] = a;
    if (nonfinite && !(fabs(a) <= 1.79769313486231570815e308)) atomicMax(nonfinite, w + 1);  // EFTB_O_CHECK_FINITE
}

// P_l(k) += bctNNLO . PctNNLOl (rows 3-5 of the NNLO block; reference parambasis.py:132-134)
__global__ __launch_bounds__(256) void reduce_nnlo_kernel(int Nx, int Nl, const double* __restrict__ biasn, const double* __restrict__ TN,
                                                          double* __restrict__ Plk, int* __restrict__ nonfinite) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y, w = blockIdx.z;
    if (k >= Nx) return;
    const double* b = biasn + (size_t)w * 3;
    const double* t = TN + (((size_t)w * Nl + l) * NROW + 3) * Nx + k;
    const double a = Plk[((size_t)w * Nl + l) * Nx + k] + (b[0] * t[0] + b[1] * t[(size_t)Nx] + b[2] * t[(size_t)2 * Nx]);
    Plk[((size_t)w * Nl + l) * Nx + k] = a;
    if (nonfinite && !(fabs(a) <= 1.79769313486231570815e308)) atomicMax(nonfinite, w + 1);
}

// ------------------------------------------------------------------------------------------------
// Analytically marginalised log-posterior (reference marginal.py:79-203, likelihood.py:483-549).
// Three launches (marg_build_kernel, one GEMM for all walkers, marg_solve_kernel).  With the coefficient rows R[g][24] (g = 0: the model at zero Gaussian parameters, g >= 1:
// its derivative with respect to Gaussian parameter g; parambasis.gaussian_rows) and the data-vector index map
//     V[g][a] = sum_r R[g][r] T[l(a)][r][x(a)]          (V[0] -= data: the residual),
//     U = C^-1 V,   G = V U^T   ((nG+1)^2 numbers),
//     F2 = G[1:,1:] + sigma^-1,  F1 = -G[1:,0] + sigma^-1 mu,  F0 = G[0,0] + mu sigma^-1 mu,
//     -2 ln P = -F1 F2^-1 F1 + F0 + ln det(F2 / 2 pi)   (LU with partial pivoting; the last term dropped with the Jeffreys option),
//     full chi2 at the best-fit Gaussian parameters b = F2^-1 F1:  G00 + 2 b.G[1:,0] + b G[1:,1:] b.
// out[w] = (ln P, full chi2, b[0..MARG_MAXG)).  det F2 <= 0 (reference: RuntimeError "det of F2ij <= 0") gives NaN.
// ------------------------------------------------------------------------------------------------
// Several tracers per likelihood point (EFTLike with tracers = [LRG, ELG, X], reference likelihood.py:483-549): the batch holds
// ntr consecutive entries per walker, the data index addresses them as one block of ntr * nl multipoles, and every entry brings
// its own coefficient rows (its bias values; zero rows for the parameters of the other tracers).
constexpr int MARG_MAXG = 24, MARG_NG1 = MARG_MAXG + 1, MARG_OUT = 2 + MARG_MAXG;

// Stage 1 of 3: V[w][g][a] (packed [walkers][nG + 1][ndata]) from the template block(s) and the coefficient rows.
__global__ __launch_bounds__(256) void marg_build_kernel(int nl, int nx, int ntr, int ndata, int nG, const int* __restrict__ index,
                                                         const double* __restrict__ data, const double* __restrict__ rows,
                                                         const double* __restrict__ T, const double* __restrict__ rowsn,
                                                         const double* __restrict__ TN, double* __restrict__ Vout) {
    // rowsn [B][MARG_NG1][3], TN: the NNLO block (with_nnlo), contributing sum_j rowsn[g][j] TN[l][3 + j][x]; both null otherwise
    extern __shared__ double sm[];
    const int ng1 = nG + 1, w = blockIdx.x, tid = threadIdx.x;
    double* R = sm;                        // [ntr][ng1][24]
    double* V = Vout + (size_t)w * ng1 * ndata;
    for (int e = tid; e < ntr * ng1 * NROW; e += 256)
        R[e] = rows[((size_t)w * ntr + e / (ng1 * NROW)) * MARG_NG1 * NROW + e % (ng1 * NROW)];
    __syncthreads();
    for (int a = tid; a < ndata; a += 256) {
        const int l = index[a] / nx, x = index[a] % nx, tr = l / nl;  // l counts the ntr * nl multipoles of the walker's entries
        const double* t = T + ((size_t)w * ntr * nl + l) * NROW * nx + x;
        const double* Rt = R + tr * ng1 * NROW;
        double tv[NROW];
#pragma unroll
        for (int r = 0; r < NROW; ++r) tv[r] = t[(size_t)r * nx];
        for (int g = 0; g < ng1; ++g) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int r = 0; r < NROW; r += 2) {
                s0 = fma(Rt[g * NROW + r], tv[r], s0);
                s1 = fma(Rt[g * NROW + r + 1], tv[r + 1], s1);
            }
            if (TN) {
                const double* tn = TN + (((size_t)w * ntr * nl + l) * NROW + 3) * nx + x;
                const double* rn = rowsn + (((size_t)w * ntr + tr) * MARG_NG1 + g) * 3;
                s0 += rn[0] * tn[0] + rn[1] * tn[(size_t)nx] + rn[2] * tn[(size_t)2 * nx];
            }
            V[(size_t)g * ndata + a] = s0 + s1 - (g == 0 ? data[a] : 0.0);
        }
    }
}

// Stage 2 is U = V C^-1 for all walkers at once on the matrix cores (gemm_rows_kernel; C^-1 is symmetric).
// Stage 3 of 3: G = V U^T per walker, then the small dense algebra.
__global__ __launch_bounds__(256) void marg_solve_kernel(int ndata, int nG, int jeffreys, const double* __restrict__ mu,
                                                         const double* __restrict__ sinv, const double* __restrict__ Vall,
                                                         const double* __restrict__ Uall, double* __restrict__ out) {
    __shared__ double G[MARG_NG1 * MARG_NG1];
    __shared__ double A[MARG_MAXG][MARG_MAXG + 1];
    __shared__ double mrow[MARG_MAXG];
    __shared__ int s_piv, s_sign;
    __shared__ double s_logdet;
    const int ng1 = nG + 1, w = blockIdx.x, tid = threadIdx.x;
    const double* V = Vall + (size_t)w * ng1 * ndata;
    const double* U = Uall + (size_t)w * ng1 * ndata;
    // G = V U^T: one wave-quarter (16 lanes) per entry, lanes stride the data index (coalesced), shuffle reduction in a fixed order
    const int sub = tid & 15, grp = tid >> 4;
    for (int e = grp; e < ng1 * ng1; e += 16) {
        const int i = e / ng1, j = e % ng1;
        double s0 = 0.0;
        for (int b = sub; b < ndata; b += 16) s0 = fma(V[(size_t)i * ndata + b], U[(size_t)j * ndata + b], s0);
        s0 += __shfl_xor(s0, 8, 16);
        s0 += __shfl_xor(s0, 4, 16);
        s0 += __shfl_xor(s0, 2, 16);
        s0 += __shfl_xor(s0, 1, 16);
        if (sub == 0) G[e] = s0;
    }
    __syncthreads();
    // F2 in LDS; LU with partial pivoting, as numpy's slogdet / solve (LAPACK getrf) in the reference: F2 may be ill-conditioned with a
    // flat prior, where a Cholesky factorisation can lose positivity to rounding although det F2 > 0.  The trailing update of every
    // step is spread over the workgroup.
    for (int e = tid; e < nG * nG; e += 256) {
        const int i = e / nG, j = e % nG;
        A[i][j] = 0.5 * (G[(i + 1) * ng1 + j + 1] + G[(j + 1) * ng1 + i + 1]) + (i == j ? sinv[i] : 0.0);
    }
    if (tid == 0) {
        s_sign = 1;
        s_logdet = 0.0;
    }
    __syncthreads();
    __shared__ int piv[MARG_MAXG];
    for (int c = 0; c < nG; ++c) {
        if (tid == 0) {
            int p = c;
            for (int i = c + 1; i < nG; ++i)
                if (fabs(A[i][c]) > fabs(A[p][c])) p = i;
            piv[c] = p;
            s_piv = p;
        }
        __syncthreads();
        const int p = s_piv;
        if (p != c && tid < nG) {
            const double t = A[c][tid];
            A[c][tid] = A[p][tid];
            A[p][tid] = t;
        }
        __syncthreads();
        const double dpiv = A[c][c];
        if (tid == 0) {
            if (p != c) s_sign = -s_sign;
            if (dpiv < 0.0) s_sign = -s_sign;
            if (dpiv == 0.0 || dpiv != dpiv) s_sign = 0;
            s_logdet += log(fabs(dpiv));
        }
        if (tid > c && tid < nG) mrow[tid] = A[tid][c] / dpiv;
        __syncthreads();
        const int n = nG - c - 1;
        for (int e = tid; e < n * n; e += 256) {
            const int i = c + 1 + e / n, j = c + 1 + e % n;
            A[i][j] = fma(-mrow[i], A[c][j], A[i][j]);
        }
        if (tid > c && tid < nG) A[tid][c] = mrow[tid];
        __syncthreads();
    }
    if (tid == 0) {
        double y[MARG_MAXG], F1[MARG_MAXG];
        double F0 = G[0];
        for (int i = 0; i < nG; ++i) {
            F1[i] = -G[(i + 1) * ng1] + sinv[i] * mu[i];
            F0 = fma(mu[i] * sinv[i], mu[i], F0);
        }
        const bool ok = s_sign > 0;
        const double logdet = s_logdet - nG * 1.8378770664093453;  // ln(2 pi) per dimension: ln det(F2 / 2 pi)
        for (int i = 0; i < nG; ++i) y[i] = F1[i];
        for (int c = 0; c < nG; ++c) {  // apply the row exchanges, then L y = P F1, U b = y
            const double t = y[c];
            y[c] = y[piv[c]];
            y[piv[c]] = t;
        }
        for (int i = 0; i < nG; ++i)
            for (int q = 0; q < i; ++q) y[i] = fma(-A[i][q], y[q], y[i]);
        for (int i = nG - 1; i >= 0; --i) {
            double t = y[i];
            for (int q = i + 1; q < nG; ++q) t = fma(-A[i][q], y[q], t);
            y[i] = t / A[i][i];  // y now holds the best-fit Gaussian parameters b = F2^-1 F1
        }
        double quad = 0.0;
        for (int i = 0; i < nG; ++i) quad = fma(F1[i], y[i], quad);  // F1 F2^-1 F1
        double full = G[0];
        for (int i = 0; i < nG; ++i) {
            full = fma(2.0 * y[i], G[(i + 1) * ng1], full);
            for (int j = 0; j < nG; ++j) full = fma(y[i] * y[j], G[(i + 1) * ng1 + j + 1], full);
        }
        const double chi2 = -quad + F0 + (jeffreys ? 0.0 : logdet);
        double* o = out + (size_t)w * MARG_OUT;
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        o[0] = ok ? -0.5 * chi2 : nan;
        o[1] = ok ? full : nan;
        for (int i = 0; i < MARG_MAXG; ++i) o[2 + i] = i < nG ? (ok ? y[i] : nan) : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------
// Many EFT parameter draws against the templates of one cosmology (the fast / slow split of reference theory.py:829-874 EFTLeaf.calculate on
// EFTLeafKernel's templates; likelihood.py:483-549, marginal.py:79-140).  Walker c (template entries c ntr ... c ntr + ntr - 1) owns the draws
// [offsets[c], offsets[c + 1]).  Everything downstream of the templates is linear in the coefficient rows, so per walker the Gram matrix
//     A_c[j][a] = T[c ntr + tau][l(a) mod nl][r][x(a)]  (column j = (tau, r); data point a of tracer tau, 0 for the other tracers),
//     A_c[J][a] = -data[a],     W_c = A_c C^-1 A_c^T   ((J + 1)^2, symmetrised; J = 24 ntr, + 3 ntr NNLO columns (tau, 3 + j) with with_nnlo)
// is built once (draws_gather_kernel, gemm_narrow_kernel, draws_gram_kernel), and a draw with rows R[tau][g][24] (+ R_n[tau][g][3]) costs
//     G = R^ W_c R^^T    (R^[g][(tau, r)] = R[tau][g][r], R^[0][J] = 1, R^[g >= 1][J] = 0)
// -- the matrix marg_solve_kernel forms as V C^-1 V^T -- and the same small algebra after it (draws_logp_kernel).
// ------------------------------------------------------------------------------------------------
constexpr int DRAW_MAXJ1 = 128;  // template columns of a walker + the data row (two column halves of 64 lanes)

// A_c [C][J1][ndata] (one workgroup per walker; lanes over the data points, as marg_build_kernel)
__global__ __launch_bounds__(256) void draws_gather_kernel(int nl, int nx, int ntr, int ndata, int J1, const int* __restrict__ index,
                                                           const double* __restrict__ data, const double* __restrict__ T,
                                                           const double* __restrict__ TN, double* __restrict__ A) {
    const int c = blockIdx.x, J = J1 - 1;
    double* Ac = A + (size_t)c * J1 * ndata;
    for (int a = threadIdx.x; a < ndata; a += 256) {
        const int l = index[a] / nx, x = index[a] % nx, tr = l / nl;  // l counts the ntr * nl multipoles of the walker's entries
        const double* t = T + ((size_t)c * ntr * nl + l) * NROW * nx + x;
        for (int tau = 0; tau < ntr; ++tau)
            for (int r = 0; r < NROW; ++r) Ac[(size_t)(tau * NROW + r) * ndata + a] = tau == tr ? t[(size_t)r * nx] : 0.0;
        if (TN) {
            const double* tn = TN + (((size_t)c * ntr * nl + l) * NROW + 3) * nx + x;
            for (int tau = 0; tau < ntr; ++tau)
                for (int j = 0; j < 3; ++j) Ac[(size_t)(ntr * NROW + 3 * tau + j) * ndata + a] = tau == tr ? tn[(size_t)j * nx] : 0.0;
        }
        Ac[(size_t)J * ndata + a] = -data[a];
    }
}

// W_c[i][j] = W_c[j][i] = (A_i . U_j + A_j . U_i) / 2 with U = A C^-1: one 16-lane group per entry i <= j, lanes stride the data index,
// shuffle reduction in a fixed order (as marg_solve_kernel)
__global__ __launch_bounds__(256) void draws_gram_kernel(int ndata, int J1, const double* __restrict__ A, const double* __restrict__ U,
                                                         double* __restrict__ W) {
    const int c = blockIdx.x, sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const double* Ac = A + (size_t)c * J1 * ndata;
    const double* Uc = U + (size_t)c * J1 * ndata;
    double* Wc = W + (size_t)c * J1 * J1;
    for (int e = blockIdx.y * 16 + grp; e < J1 * J1; e += gridDim.y * 16) {
        const int i = e / J1, j = e % J1;
        if (i > j) continue;  // (uniform over the 16-lane group: the shuffles stay inside it)
        double s0 = 0.0, s1 = 0.0;
        for (int b = sub; b < ndata; b += 16) {
            s0 = fma(Ac[(size_t)i * ndata + b], Uc[(size_t)j * ndata + b], s0);
            s1 = fma(Ac[(size_t)j * ndata + b], Uc[(size_t)i * ndata + b], s1);
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            s0 += __shfl_xor(s0, m, 16);
            s1 += __shfl_xor(s1, m, 16);
        }
        if (sub == 0) {
            const double w = 0.5 * (s0 + s1);
            Wc[(size_t)i * J1 + j] = w;
            Wc[(size_t)j * J1 + i] = w;
        }
    }
}

// LDS written by some lanes of a wave and read by others: no workgroup barrier, only the wave's own order
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// R^[h][j] of draw Rd / Rn (column j: (tau, r) for j < 24 ntr, NNLO (tau, jj) after them, the data row at J)
__device__ __forceinline__ double draw_coef(const double* Rd, const double* Rn, int ntr, int ng1, int J, int h, int j) {
    if (j < ntr * NROW) return Rd[((j / NROW) * ng1 + h) * NROW + j % NROW];
    if (j < J) {
        const int jn = j - ntr * NROW;
        return Rn ? Rn[((jn / 3) * ng1 + h) * 3 + jn % 3] : 0.0;
    }
    return h == 0 ? 1.0 : 0.0;
}

// The small algebra of one draw after G = R^ W_c R^^T (one wave; G [nG + 1][nG + 1] in the wave's LDS), and the [MARG_OUT] record of the
// draw.  Every logp draw kernel calls this one function, so the record of a draw has the same bits whichever call computed it.
// F2 = sym(G[1:,1:]) + sigma^-2, F1 and F0 as marg_solve_kernel; LU with partial pivoting wave-synchronously: lane i keeps row i of F2,
// augmented with F1[i], in registers; the pivot row is broadcast with v_readlane.  The rows are not exchanged: `pos` is the place the
// row would hold in a row-exchanging LU (pivot choice on ties and the sign of det follow it), the right-hand side is eliminated with the
// rows (= marg_solve_kernel's forward substitution, same operations in the same order), then back substitution column by column.
// With ADJ (the gradient kernel), lane i also carries row i of the identity.  The multiplier of every eliminated row is kept in the
// place of the entry it clears (a[c2] of a row below place c2, which nothing reads again), so the rows hold L and U of the pivoted F2.
// Unless Jeffreys (wave-uniform: S = v v^T needs no inverse), the identity is then eliminated and substituted back with the same
// steps, ADJ_KB columns at a time (independent chains; lane i starts with e_k[i] = [i == k]): element c2 of column k of F2^-1 ends in the
// lane whose row holds place c2.  S is written over G (dead by then) in the wave's LDS:
//   S[0][0] = 1, S[0][1 + k] = S[1 + k][0] = b[k], S[1 + i][1 + k] = b[i] b[k] + [not Jeffreys] F2^-1[i][k].
// -> ok (det F2 > 0), wave-uniform
constexpr int ADJ_KB = 4;

// With HESS (the Hessian kernel; needs ADJ), F2^-1 is taken under Jeffreys too and also written to Ks [nG][nG] (row: the place, as S).
template <bool ADJ, bool HESS = false>
__device__ __forceinline__ bool draws_solve(int lane, int nG, int jeffreys, double* Gs, const double* mu, const double* sinv, double* o,
                                            double* Ks = nullptr) {
    const int ng1 = nG + 1;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    // ---- F2 | F1 per lane (row i = lane), LU with partial pivoting
    const bool own = lane < nG;
    double a[MARG_MAXG], aug = 0.0;
#pragma unroll
    for (int j = 0; j < MARG_MAXG; ++j)
        a[j] = (own && j < nG) ? 0.5 * (Gs[(lane + 1) * ng1 + j + 1] + Gs[(j + 1) * ng1 + lane + 1]) + (lane == j ? sinv[j] : 0.0) : 0.0;
    if (own) aug = -Gs[(lane + 1) * ng1] + sinv[lane] * mu[lane];
    const double f1 = aug;
    int pos = lane, sgn = 1;
    double logdet = 0.0, dpv[MARG_MAXG];
    int pl[MARG_MAXG];
#pragma unroll
    for (int c2 = 0; c2 < MARG_MAXG; ++c2) {
        if (c2 >= nG) continue;
        // pivot: largest |F2[i][c2]| among the rows not yet eliminated, the first in row order on ties (marg_solve_kernel, LAPACK)
        const bool cand = own && pos >= c2;
        double v = fabs(a[c2]);
        if (!(v >= 0.0)) v = -0.5;  // NaN: a total order keeps the reduction's result the same in every lane
        if (!cand) v = -1.0;
        int kp = cand ? pos : 1 << 20, who = lane;
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {  // lanes 0-31 hold every row (nG <= 24)
            const double v2 = __shfl_xor(v, m);
            const int k2 = __shfl_xor(kp, m), w2 = __shfl_xor(who, m);
            if (v2 > v || (v2 == v && k2 < kp)) {
                v = v2;
                kp = k2;
                who = w2;
            }
        }
        const int p = __builtin_amdgcn_readlane(who, 0);
        const int pp = __builtin_amdgcn_readlane(pos, p);
        if (pp != c2) sgn = -sgn;
        if (pos == c2) pos = pp;  // the row at place c2 takes the pivot row's place
        if (lane == p) pos = c2;
        const double dpiv = readlane_f64(a[c2], p);
        if (dpiv < 0.0) sgn = -sgn;
        if (dpiv == 0.0 || dpiv != dpiv) sgn = 0;
        logdet += log(fabs(dpiv));
        dpv[c2] = dpiv;
        pl[c2] = p;
        const bool elim = own && pos > c2;
        const double m = elim ? a[c2] / dpiv : 0.0;
#pragma unroll
        for (int j = c2 + 1; j < MARG_MAXG; ++j)
            if (j < nG) {
                const double u = readlane_f64(a[j], p);
                if (elim) a[j] = fma(-m, u, a[j]);
            }
        const double yc = readlane_f64(aug, p);
        if (elim) aug = fma(-m, yc, aug);
        if (ADJ && elim) a[c2] = m;  // (L: the cleared entry is not read again)
    }
    // back substitution U b = y: b = F2^-1 F1, the best-fit Gaussian parameters
    double b[MARG_MAXG];
#pragma unroll
    for (int c2 = MARG_MAXG - 1; c2 >= 0; --c2) {
        b[c2] = 0.0;
        if (c2 < nG) {
            const double bc = readlane_f64(aug, pl[c2]) / dpv[c2];
            b[c2] = bc;
            if (own && pos < c2) aug = fma(-a[c2], bc, aug);
        }
    }
    // F1 F2^-1 F1, F0 and the full chi2 at b (row sums per lane, added in row order)
    double bi = 0.0, srow = 0.0;
#pragma unroll
    for (int j = 0; j < MARG_MAXG; ++j)
        if (j < nG) {
            if (lane == j) bi = b[j];
            if (own) srow = fma(b[j], Gs[(lane + 1) * ng1 + j + 1], srow);
        }
    const double trow = own ? bi * fma(2.0, Gs[(lane + 1) * ng1], srow) : 0.0;
    double quad = 0.0, F0 = Gs[0], full = Gs[0];
#pragma unroll
    for (int i = 0; i < MARG_MAXG; ++i)
        if (i < nG) {
            quad = fma(readlane_f64(f1, i), b[i], quad);
            F0 = fma(mu[i] * sinv[i], mu[i], F0);
            full += readlane_f64(trow, i);
        }
    const bool ok = sgn > 0;
    const double chi2 = -quad + F0 + (jeffreys ? 0.0 : logdet - nG * 1.8378770664093453);  // ln det(F2 / 2 pi)
    if (lane == 0) {
        o[0] = ok ? -0.5 * chi2 : nan;
        o[1] = ok ? full : nan;
    }
    if (lane < MARG_MAXG) o[2 + lane] = own ? (ok ? bi : nan) : 0.0;
    if constexpr (ADJ) {
        // ---- S over G: lane i < nG writes row 1 + pos, lane nG row 0
        wave_lds_sync();  // (every read of G is done)
        double bp = 0.0;
#pragma unroll
        for (int j = 0; j < MARG_MAXG; ++j)
            if (j < nG && pos == j) bp = b[j];
        double* srw = Gs + (own ? pos + 1 : 0) * ng1;
        if (lane <= nG) {
            srw[0] = own ? bp : 1.0;
#pragma unroll
            for (int k = 0; k < MARG_MAXG; ++k)
                if (k < nG) srw[1 + k] = own ? bp * b[k] : b[k];
        }
        if (HESS || !jeffreys) {
            double rdp[MARG_MAXG];
#pragma unroll
            for (int c2 = 0; c2 < MARG_MAXG; ++c2) rdp[c2] = c2 < nG ? 1.0 / dpv[c2] : 0.0;
            for (int k0 = 0; k0 < nG; k0 += ADJ_KB) {
                double y[ADJ_KB];
#pragma unroll
                for (int q = 0; q < ADJ_KB; ++q) y[q] = lane == k0 + q ? 1.0 : 0.0;
#pragma unroll
                for (int c2 = 0; c2 < MARG_MAXG; ++c2)
                    if (c2 < nG) {
                        const bool below = own && pos > c2;
#pragma unroll
                        for (int q = 0; q < ADJ_KB; ++q) {
                            const double yc = readlane_f64(y[q], pl[c2]);
                            if (below) y[q] = fma(-a[c2], yc, y[q]);
                        }
                    }
#pragma unroll
                for (int c2 = MARG_MAXG - 1; c2 >= 0; --c2)
                    if (c2 < nG) {
                        const bool above = own && pos < c2;
#pragma unroll
                        for (int q = 0; q < ADJ_KB; ++q) {
                            const double xc = readlane_f64(y[q], pl[c2]) * rdp[c2];
                            if (above) y[q] = fma(-a[c2], xc, y[q]);
                            if (pos == c2) y[q] = xc;
                        }
                    }
#pragma unroll
                for (int q = 0; q < ADJ_KB; ++q)
                    if (own && k0 + q < nG) {
                        if (!HESS || !jeffreys) srw[1 + k0 + q] += y[q];
                        if constexpr (HESS) Ks[pos * nG + k0 + q] = y[q];
                    }
            }
        }
    }
    return ok;
}

constexpr int RECIPE_MAXP = 32, RECIPE_MAXTERMS = 1024, RECIPE_FPOW = 7, RECIPE_MAXTR = 8;  // (draw recipes: see RecipeTab)
constexpr int CHAIN_PRI = 4 * RECIPE_MAXP;                                                 // the prior table of the chain kernel
// the ensemble kernel: members of an ensemble and waves of its workgroup at most, and a member's slot in the ensemble area of the LDS,
// theta [RECIPE_MAXP] | record [MARG_OUT] | ln P | pri | accept count
constexpr int ENS_MAXK = 64, ENS_MAXW = 8, ENS_REC = RECIPE_MAXP, ENS_LP = ENS_REC + MARG_OUT, ENS_PRI = ENS_LP + 1, ENS_NA = ENS_PRI + 1, ENS_SLOT = ENS_NA + 1;

// The dynamic LDS of a draw kernel, in doubles: what the host sizes the launch from and what the kernel takes its pointers from.
//   per workgroup  W_c [J1][J1] at 0, then (all but rows) fp [RECIPE_MAXTR][RECIPE_FPOW] and the int tables, two ints to a double:
//                  col [nnzp]; erow [nnzp] (gradient, Hessian, sample); drow | dcol [ndtp] (Hessian); then pr [CHAIN_PRI] (chain, drag).
//                  drag stages a pair of walkers: the end walker's W_c [J1][J1] behind the start walker's (at W2(J1)) and its fp behind fp (at fp2())
//   per wave       (all but rows) th [P + 1 -> 34], val [nnzp]; H [ng1][J1], G [ng1][ng1]; then the kind's tail:
//                  Hessian K [nG][nG] | dval [ndtp] | hv [J1] | u [P][nG] | w [P][nG] | G_p | M_p [P][nG][nG] (the last two empty under Jeffreys)
//                  sample  bs [ADJ_KB][nG]
//                  chain   tc | tp [RECIPE_MAXP] (the current and the trial theta) | rs [2][MARG_OUT] (two records)
//                  drag    tc | tp as chain | rs [2][2][MARG_OUT] (two pairs of records, start | end walker in each)
//                  hmc     tc | tp | rs as chain | gs [2][RECIPE_MAXP] (the gradients of the two records) | mo [RECIPE_MAXP] (the momentum)
//                          | F [P][P] (the chain's factor); erow is staged as for the gradient
//   ensemble       (the ensemble kernel alone, behind the parts of its nw waves of the chain kind, at ens(nw)) K slots of ENS_SLOT doubles
// nnzp and ndtp: the entries of the recipe and its derivative records, rounded up to even.  A region a kind does not have is empty.
enum DrawKind { DRAW_ROWS, DRAW_PARAMS, DRAW_GRAD, DRAW_HESS, DRAW_SAMPLE, DRAW_CHAIN, DRAW_DRAG, DRAW_HMC };

struct DrawLds {
    int fp = 0, col = 0, erow = 0, drow = 0, dcol = 0, pr = 0, wg = 0;  // offsets from the start of the LDS; wg: doubles per workgroup
    int th = 0, val = 0, H = 0, G = 0, K = 0, dval = 0, hv = 0, u = 0, w = 0, Gp = 0, Mp = 0, bs = 0, tc = 0, tp = 0, rs = 0,
        wave = 0;  // offsets from the start of the wave's part; wave: doubles per wave
    int gs = 0, mo = 0, F = 0;  // (hmc: between rs and the end of the wave's part)

    DrawLds() = default;
    static constexpr bool has_erow(DrawKind kind) { return kind == DRAW_GRAD || kind == DRAW_HESS || kind == DRAW_SAMPLE || kind == DRAW_HMC; }
    // (every kind but DRAW_DRAG, whose layout is drag() below: of() is the way in that knows all eight)
    __host__ __device__ constexpr DrawLds(DrawKind kind, int J1, int nG, int nnz, int ndt, int P, int jeffreys) {
#ifndef __HIP_DEVICE_COMPILE__
        if (kind == DRAW_DRAG) abort();  // a constant expression that gets here does not compile; the kernels name their kind and never do
#endif
        const bool recipe = kind != DRAW_ROWS, adj = has_erow(kind), hess = kind == DRAW_HESS, hmc = kind == DRAW_HMC, chain = kind == DRAW_CHAIN || hmc;
        const int ng1 = nG + 1, nnzp = (nnz + 1) & ~1, ndtp = (ndt + 1) & ~1, gpn = hess && !jeffreys ? P * nG * nG : 0;
        int o = J1 * J1;
        fp = o, o += recipe ? RECIPE_MAXTR * RECIPE_FPOW : 0;
        col = o, o += recipe ? nnzp / 2 : 0;
        erow = o, o += adj ? nnzp / 2 : 0;
        drow = o, o += hess ? ndtp / 2 : 0;
        dcol = o, o += hess ? ndtp / 2 : 0;
        pr = o, o += chain ? CHAIN_PRI : 0;
        wg = o;
        o = 0;
        th = o, o += recipe ? 34 : 0;
        val = o, o += recipe ? nnzp : 0;
        H = o, o += ng1 * J1;
        G = o, o += ng1 * ng1;
        K = o, o += hess ? nG * nG : 0;
        dval = o, o += hess ? ndtp : 0;
        hv = o, o += hess ? J1 : 0;
        u = o, o += hess ? P * nG : 0;
        w = o, o += hess ? P * nG : 0;
        Gp = o, o += gpn;
        Mp = o, o += gpn;
        bs = o, o += kind == DRAW_SAMPLE ? ADJ_KB * nG : 0;
        tc = o, o += chain ? RECIPE_MAXP : 0;
        tp = o, o += chain ? RECIPE_MAXP : 0;
        rs = o, o += chain ? 2 * MARG_OUT : 0;
        gs = o, o += hmc ? 2 * RECIPE_MAXP : 0;
        mo = o, o += hmc ? RECIPE_MAXP : 0;
        F = o, o += hmc ? P * P : 0;
        wave = o;
    }
    // DRAW_DRAG: the chain kind's layout with room for the end walker -- its W_c behind the start walker's (at W2(J1)), its powers of f
    // behind fp (at fp2()), and a second pair of records at the end of the wave's part.  Built beside the constructor, not in it: the
    // other kinds' kernels compile from the same expressions as before
    static __host__ __device__ constexpr DrawLds drag(int J1, int nG, int nnz, int P, int jeffreys) {
        DrawLds L(DRAW_CHAIN, J1, nG, nnz, 0, P, jeffreys);
        const int more = J1 * J1 + RECIPE_MAXTR * RECIPE_FPOW;
        L.fp += J1 * J1;
        L.col += more, L.erow += more, L.drow += more, L.dcol += more, L.pr += more, L.wg += more;
        L.wave += 2 * MARG_OUT;
        L.gs += 2 * MARG_OUT, L.mo += 2 * MARG_OUT, L.F += 2 * MARG_OUT;  // (empty, at the end of the wave's part)
        return L;
    }
    static __host__ __device__ constexpr DrawLds of(DrawKind kind, int J1, int nG, int nnz, int ndt, int P, int jeffreys) {
        return kind == DRAW_DRAG ? drag(J1, nG, nnz, P, jeffreys) : DrawLds(kind, J1, nG, nnz, ndt, P, jeffreys);
    }
    static __host__ __device__ constexpr int W2(int J1) { return J1 * J1; }
    __host__ __device__ constexpr int fp2() const { return fp + RECIPE_MAXTR * RECIPE_FPOW; }
    __host__ __device__ constexpr size_t bytes_wg() const { return (size_t)wg * sizeof(double); }
    __host__ __device__ constexpr size_t bytes_wave() const { return (size_t)wave * sizeof(double); }
    __host__ __device__ constexpr size_t bytes(int nw) const { return bytes_wg() + nw * bytes_wave(); }
    // the ensemble area of the ensemble kernel (chain kind): where it starts behind nw waves, the bytes of a launch with K members, and the
    // waves of a workgroup, min(ENS_MAXW, K / 2, as many as fit beside W_c and the area); 0 if one does not
    __host__ __device__ constexpr int ens(int nw) const { return wg + nw * wave; }
    __host__ __device__ constexpr size_t bytes_ens(int nw, int K) const { return bytes(nw) + (size_t)K * ENS_SLOT * sizeof(double); }
    __host__ __device__ constexpr int fit_ens(int K, size_t limit) const {
        int nw = 0;
        while (nw < ENS_MAXW && 2 * (nw + 1) <= K && bytes_ens(nw + 1, K) <= limit) ++nw;
        return nw;
    }
    // the waves of a workgroup: 4, 2 or 1, as many as fit beside W_c (drag: beside both); 0 if one does not
    __host__ __device__ constexpr int fit(size_t limit) const { return bytes(4) <= limit ? 4 : bytes(2) <= limit ? 2 : bytes(1) <= limit ? 1 : 0; }
    // every region holds what its kernel keeps there and ends where the next begins or before (the int tables in whole doubles, so every
    // region starts on an 8-byte boundary), whatever the arithmetic above becomes
    __host__ __device__ constexpr bool sound(DrawKind kind, int J1, int nG, int nnz, int ndt, int P, int jeffreys) const {
        const bool recipe = kind != DRAW_ROWS, adj = has_erow(kind), hess = kind == DRAW_HESS;
        const bool drag = kind == DRAW_DRAG, hmc = kind == DRAW_HMC, chain = kind == DRAW_CHAIN || drag || hmc;
        const int ng1 = nG + 1, gpn = hess && !jeffreys ? P * nG * nG : 0;
        const int at[] = {0, drag ? W2(J1) : fp, fp, drag ? fp2() : col, col, erow, drow, dcol, pr, wg},
                  atw[] = {th, val, H, G, K, dval, hv, u, w, Gp, Mp, bs, tc, tp, rs, gs, mo, F, wave};
        const int len[] = {J1 * J1, drag ? J1 * J1 : 0, recipe ? RECIPE_MAXTR * RECIPE_FPOW : 0, drag ? RECIPE_MAXTR * RECIPE_FPOW : 0, recipe ? (nnz + 1) / 2 : 0,
                           adj ? (nnz + 1) / 2 : 0, hess ? (ndt + 1) / 2 : 0, hess ? (ndt + 1) / 2 : 0, chain ? CHAIN_PRI : 0};
        const int lenw[] = {recipe ? P + 1 : 0, recipe ? nnz : 0, ng1 * J1, ng1 * ng1, hess ? nG * nG : 0, hess ? ndt : 0, hess ? J1 : 0, hess ? P * nG : 0,
                            hess ? P * nG : 0, gpn, gpn, kind == DRAW_SAMPLE ? ADJ_KB * nG : 0, chain ? P : 0, chain ? P : 0, drag ? 4 * MARG_OUT : chain ? 2 * MARG_OUT : 0,
                            hmc ? RECIPE_MAXP + P : 0, hmc ? P : 0, hmc ? P * P : 0};
        for (int i = 0; i < 9; ++i)
            if (at[i] + len[i] > at[i + 1]) return false;
        for (int i = 0; i < 18; ++i)
            if (atw[i] + lenw[i] > atw[i + 1]) return false;
        return true;
    }
};

// The layout is pinned on the published figures of the largest shape there is (J + 1 = 121, nG = 24, 1024 recipe entries, one wave)
// and on `sound` at that shape and at an odd one, with Jeffreys off and on
constexpr size_t draw_lds_pin(DrawKind kind, int nnz) { return DrawLds(kind, 121, 24, nnz, 0, RECIPE_MAXP, 0).bytes(1); }
static_assert(MARG_OUT == 26 && ADJ_KB == 4, "the figures below are for these");
static_assert(draw_lds_pin(DRAW_ROWS, 1024) == 146328 && draw_lds_pin(DRAW_PARAMS, 1024) == 159336 && draw_lds_pin(DRAW_GRAD, 1024) == 163432 &&
                  draw_lds_pin(DRAW_CHAIN, 1024) == 161288,
              "DrawLds: rows, params, gradient, chain at the largest shape");
static_assert(draw_lds_pin(DRAW_SAMPLE, 1024) == 147816 + 16 * 1024 && draw_lds_pin(DRAW_SAMPLE, 999) == 147816 + 16 * 1000 &&
                  draw_lds_pin(DRAW_SAMPLE, 1000) == 163816,
              "DrawLds: sample, 147816 + 16 nnzp bytes");
// drag, which holds two Gram matrices, at the largest shape that fits: three tracers with NNLO (J + 1 = 82), nG = 24, 1024 recipe entries, one
// wave; four tracers at nG = 24 (J + 1 = 97) do not fit
static_assert(DrawLds::drag(82, 24, 1024, RECIPE_MAXP, 0).bytes(1) == 144808 && DrawLds::drag(82, 24, 1024, RECIPE_MAXP, 0).fit(160 * 1024) == 1 &&
                  DrawLds::drag(97, 24, 0, 1, 0).fit(160 * 1024) == 0,
              "DrawLds: drag at J + 1 = 82 and 97");
// hmc, which adds erow, two gradients, the momentum and F [P][P] to the chain kind, at the largest shape that fits: four tracers
// with NNLO (J + 1 = 109), nG = 24, 1024 recipe entries, P = 32, one wave; five tracers (J + 1 = 121) at that nG and recipe do not
static_assert(DrawLds(DRAW_HMC, 109, 24, 1024, 0, RECIPE_MAXP, 0).bytes(1) == 149864 && DrawLds(DRAW_HMC, 109, 24, 1024, 0, RECIPE_MAXP, 0).fit(160 * 1024) == 1 &&
                  DrawLds(DRAW_HMC, 121, 24, 1024, 0, 1, 0).fit(160 * 1024) == 0,
              "DrawLds: hmc at J + 1 = 109 and 121");
// the ensemble area: 61 doubles per member; at the largest shape four members beside one wave, at the fixtures' (J + 1 = 25, nG = 3) eight
// waves beside ENS_MAXK members
static_assert(ENS_SLOT == 61 && DrawLds(DRAW_CHAIN, 121, 24, 1024, 0, RECIPE_MAXP, 0).fit_ens(4, 160 * 1024) == 1 &&
                  DrawLds(DRAW_CHAIN, 121, 24, 1024, 0, RECIPE_MAXP, 0).fit_ens(6, 160 * 1024) == 0 &&
                  DrawLds(DRAW_CHAIN, 25, 3, 37, 0, 5, 0).fit_ens(ENS_MAXK, 160 * 1024) == 8 && DrawLds(DRAW_CHAIN, 25, 3, 37, 0, 5, 0).fit_ens(6, 160 * 1024) == 3,
              "DrawLds: the ensemble area");
constexpr bool draw_lds_sound(int J1, int nG, int nnz, int ndt, int P) {
    for (int kind = DRAW_ROWS; kind <= DRAW_HMC; ++kind)
        for (int jeffreys = 0; jeffreys < 2; ++jeffreys)
            if (!DrawLds::of((DrawKind)kind, J1, nG, nnz, ndt, P, jeffreys).sound((DrawKind)kind, J1, nG, nnz, ndt, P, jeffreys)) return false;
    return true;
}
static_assert(draw_lds_sound(121, 24, 1024, 2048, RECIPE_MAXP) && draw_lds_sound(25, 3, 37, 51, 5) && draw_lds_sound(2, 0, 0, 0, 0),
              "DrawLds: a region overlaps the next");

// One workgroup per (walker, share of its draws): W_c is staged in LDS once, then every wave takes one draw at a time.
//   H = R^ W_c    lanes over the columns j (j = lane and lane + 64 with TWO), nG + 1 accumulators each; R^[g][k] wave-uniform (scalar loads)
//   G = H R^^T    lane h (lanes 32-63: the second half of the j sum, added with one shuffle), H from the wave's LDS scratch, G back to it
//   then draws_solve on G
// Output: the [MARG_OUT] record of the LOGP stage per draw.  LDS: DrawLds, DRAW_ROWS.
template <bool TWO>
__global__ __launch_bounds__(256) void draws_logp_kernel(int ntr, int nG, int J1, int jeffreys, const long long* __restrict__ offsets,
                                                         const double* __restrict__ rows, const double* __restrict__ rowsn,
                                                         const double* __restrict__ W, const double* __restrict__ mu,
                                                         const double* __restrict__ sinv, double* __restrict__ out) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng1 = nG + 1, J = J1 - 1;
    const long long d0 = offsets[c], d1 = offsets[c + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;  // (workgroup-uniform: no draw for this share)
    const DrawLds L(DRAW_ROWS, J1, nG, 0, 0, 0, jeffreys);
    double* Ws = sm;
    for (int e = threadIdx.x; e < J1 * J1; e += blockDim.x) Ws[e] = W[(size_t)c * J1 * J1 + e];
    __syncthreads();
    double* Hs = sm + L.wg + wv * L.wave + L.H;
    double* Gs = sm + L.wg + wv * L.wave + L.G;
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        const double* Rd = rows + (size_t)d * ntr * ng1 * NROW;
        const double* Rn = rowsn ? rowsn + (size_t)d * ntr * ng1 * 3 : nullptr;
        // ---- H = R^ W_c
        double h0[MARG_NG1], h1[MARG_NG1];
#pragma unroll
        for (int g = 0; g < MARG_NG1; ++g) h0[g] = h1[g] = 0.0;
        const bool c0 = lane < J1, c1 = TWO && lane + 64 < J1;
        const int kn = Rn ? J : ntr * NROW;  // (no NNLO rows: those columns have zero coefficients)
        for (int k = 0; k < kn; ++k) {
            const bool main = k < ntr * NROW;
            const int tau = main ? k / NROW : (k - ntr * NROW) / 3, r = main ? k % NROW : (k - ntr * NROW) % 3, stride = main ? NROW : 3;
            const double* rk = main ? Rd + tau * ng1 * NROW + r : Rn + tau * ng1 * 3 + r;
            const double w0 = c0 ? Ws[k * J1 + lane] : 0.0, w1 = c1 ? Ws[k * J1 + 64 + lane] : 0.0;
#pragma unroll
            for (int g = 0; g < MARG_NG1; ++g)
                if (g < ng1) {
                    const double rv = rk[g * stride];
                    h0[g] = fma(rv, w0, h0[g]);
                    if (TWO) h1[g] = fma(rv, w1, h1[g]);
                }
        }
        h0[0] += c0 ? Ws[J * J1 + lane] : 0.0;  // the data row: R^[0][J] = 1
        if (TWO) h1[0] += c1 ? Ws[J * J1 + 64 + lane] : 0.0;
#pragma unroll
        for (int g = 0; g < MARG_NG1; ++g)
            if (g < ng1) {
                if (c0) Hs[g * J1 + lane] = h0[g];
                if (c1) Hs[g * J1 + 64 + lane] = h1[g];
            }
        wave_lds_sync();
        // ---- G = H R^^T: lane h sums j in [0, Jh), lane 32 + h in [Jh, J1)
        {
            const int h = lane & 31, half = lane >> 5, Jh = (J1 + 1) >> 1;
            const bool hl = h < ng1;
            double acc[MARG_NG1];
#pragma unroll
            for (int g = 0; g < MARG_NG1; ++g) acc[g] = 0.0;
            for (int q = 0; q < Jh; ++q) {
                const int j = half * Jh + q;
                const bool jl = j < J1;
                const double rv = (hl && jl) ? draw_coef(Rd, Rn, ntr, ng1, J, h, j) : 0.0;
                const int jj = jl ? j : 0;
#pragma unroll
                for (int g = 0; g < MARG_NG1; ++g)
                    if (g < ng1) acc[g] = fma(Hs[g * J1 + jj], rv, acc[g]);
            }
#pragma unroll
            for (int g = 0; g < MARG_NG1; ++g)
                if (g < ng1) {
                    acc[g] += __shfl_xor(acc[g], 32);
                    if (half == 0 && hl) Gs[g * ng1 + h] = acc[g];
                }
        }
        wave_lds_sync();
        draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, out + (size_t)d * MARG_OUT);
        wave_lds_sync();  // (the next draw overwrites H and G)
    }
}

// P_d[tau][l][x] = sum_r b_d[tau][r] T[c ntr + tau][l][r][x] (+ sum_j bn_d[tau][j] TN[c ntr + tau][l][3 + j][x]) for the draws of walker c:
// the templates of one (walker, tracer, l, 64-wide x tile) stay in registers, the waves of the workgroup take the draws in turn, and the
// coefficients are wave-uniform loads.  The same two FMA chains split at msplit as reduce_kernel, then the NNLO sum as reduce_nnlo_kernel:
// the same bits.  Write-bound (8 nl nx bytes per draw and tracer).
__global__ __launch_bounds__(256) void draws_reduce_kernel(int nx, int nl, int ntr, int msplit, int xtiles, const long long* __restrict__ offsets,
                                                           const double* __restrict__ bias, const double* __restrict__ T,
                                                           const double* __restrict__ biasn, const double* __restrict__ TN,
                                                           double* __restrict__ plk) {
    const int tile = blockIdx.x % xtiles, share = blockIdx.x / xtiles, nshare = gridDim.x / xtiles;
    const int tau = blockIdx.y / nl, l = blockIdx.y % nl, c = blockIdx.z;
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x = tile * 64 + lane;
    const bool live = x < nx;
    const size_t ent = (size_t)c * ntr + tau;
    const double* t = T + (ent * nl + l) * NROW * nx + (live ? x : 0);
    double tv[NROW], tn[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < NROW; ++r) tv[r] = t[(size_t)r * nx];
    if (TN) {
        const double* u = TN + ((ent * nl + l) * NROW + 3) * nx + (live ? x : 0);
#pragma unroll
        for (int j = 0; j < 3; ++j) tn[j] = u[(size_t)j * nx];
    }
    const long long d1 = offsets[c + 1];
    for (long long d = offsets[c] + (long long)share * nw + wv; d < d1; d += (long long)nshare * nw) {
        const double* b = bias + ((size_t)d * ntr + tau) * NROW;
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int r = 0; r < NROW; ++r) {
            if (r < msplit) a0 = fma(b[r], tv[r], a0);
            else a1 = fma(b[r], tv[r], a1);
        }
        double a = a0 + a1;
        if (TN) {
            const double* bn = biasn + ((size_t)d * ntr + tau) * 3;
            a = a + (bn[0] * tn[0] + bn[1] * tn[1] + bn[2] * tn[2]);
        }
        if (live) plk[(((size_t)d * ntr + tau) * nl + l) * nx + x] = a;
    }
}

// ------------------------------------------------------------------------------------------------
// Window precompute (reference window.py:262-359).  tables.py window_tables collapses the reference's per-(a, l, k)
// FFTLog(4096) + power-law sum into  W_al(k, p) = sum_i Qt_al[i] j_{2a}(k x_i) T_l[i][p]:  window_bessel_kernel writes the
// left factor A[a][l][k][i] = Qt_al[i] j_{2a}(k x_i), gemm_rows_kernel multiplies it with T_l on the matrix cores (one launch
// per l, rows = (a, k)), window_maskdp_kernel applies the |p - k| < windowk band and the trapezoid dp weights, and a last
// gemm_rows_kernel folds the k -> p cubic spline in (Wfold = Waldk S), so Window.Window is one dense operator.
// ------------------------------------------------------------------------------------------------
// spherical Bessel j_0, j_2, j_4: ascending series below x = 4 (the closed forms cancel like x^-(2n+1) there), upward
// recurrence from sin / cos above (stable for x > n)
__device__ inline void sph_j024(double x, double j[3]) {
    if (x < 4.0) {
        const double h = -0.5 * x * x;
        const double lead[3] = {1.0, x * x / 15.0, x * x * x * x / 945.0};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int n = 2 * a;
            double t = 1.0, sum = 1.0;
#pragma unroll 4
            for (int m = 1; m <= 24; ++m) {
                t *= h / (double)(m * (2 * n + 2 * m + 1));
                sum += t;
            }
            j[a] = lead[a] * sum;
        }
    } else {
        double sn, cs;
        sincos(x, &sn, &cs);
        const double r = 1.0 / x;
        const double j0 = sn * r, j1 = (sn * r - cs) * r;
        const double j2 = 3.0 * r * j1 - j0, j3 = 5.0 * r * j2 - j1;
        j[0] = j0; j[1] = j2; j[2] = 7.0 * r * j3 - j2;
    }
}

__global__ __launch_bounds__(256) void window_bessel_kernel(int Na, int Nl, int Nk, int nx, const double* __restrict__ k,
                                                            const double* __restrict__ x, const double* __restrict__ Qt,
                                                            double* __restrict__ A) {
    const int i = blockIdx.x * 256 + threadIdx.x, kk = blockIdx.y;
    if (i >= nx || kk >= Nk) return;
    double j[3];
    sph_j024(k[kk] * x[i], j);
    for (int a = 0; a < Na; ++a)
        for (int l = 0; l < Nl; ++l) A[(((size_t)a * Nl + l) * Nk + kk) * nx + i] = Qt[((size_t)a * Nl + l) * nx + i] * j[a];
}

// Waldk[r][k][p] = Wal[r][k][p] * [k - windowk < p < k + windowk] * (p_p - p_{p-1})   (reference window.py:348-359), r = (a, l)
__global__ __launch_bounds__(256) void window_maskdp_kernel(int R, int Nk, int Np, const double* __restrict__ k, const double* __restrict__ p,
                                                            int withmask, double windowk, const double* __restrict__ Wal,
                                                            double* __restrict__ Waldk) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)R * Nk * Np) return;
    const int ip = (int)(idx % Np), ik = (int)((idx / Np) % Nk);
    const double pv = p[ip], kv = k[ik];
    const double dp = ip ? pv - p[ip - 1] : 0.0;
    const bool in = !withmask || (pv < kv + windowk && pv > kv - windowk);
    Waldk[idx] = in ? Wal[idx] * dp : 0.0;
}

// ------------------------------------------------------------------------------------------------
// FP64 MFMA issue-rate microbenchmark (roofline denominator): NACC independent accumulator chains.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void mfma_peak_kernel(int iters, double* sink) {
    v4d acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    const double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) sink[0] = s;
}

// ------------------------------------------------------------------------------------------------
// Streaming-read calibration for the FETCH_SIZE counter: every lane reads W consecutive doubles per trip (W = 1: the 8 B/lane pattern of
// the template kernels here; W = 2: the 16 B/lane pattern MI355X_MICROARCH.md calibrated), a known byte count per launch.
// ------------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void stream_read_kernel(const double* __restrict__ src, size_t n, double* sink) {
    double s = 0.0;
    const size_t stride = (size_t)gridDim.x * blockDim.x * W;
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * W; i + W <= n; i += stride) {
        if (W == 1) s += __builtin_nontemporal_load(src + i);
        else {
            const v2d v = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(src + i));
            s += v[0] + v[1];
        }
    }
    if (s == 12345.678) sink[0] = s;
}

// ------------------------------------------------------------------------------------------------
// Draws given as EFT parameter values: the rows are built on the device from a draw recipe (eftb_set_draw_recipe).  Entry n of the recipe
// is one non-zero (row g, tracer tau, column r) of R^, the sum of its terms coef * f[tau]^e * theta[i] * theta[j] * theta[k]; the entries
// are sorted by (g, tau, r) and the terms of an entry keep a fixed order, so a draw's sum does not depend on how the work is split.
//   tab = rowstart [ng1 + 1] (first entry of row g) | ent [nnz] (tau * 32 + r) | tstart [nnz + 1] (first term of entry n) | pack [nterms]
//         | slot [ntr * 27] (the entry of (tau, r) in row 0, or -1: draws_recipe_rows_kernel)
//   pack = i | j << 6 | k << 12 | (tau * 7 + e) << 18, with the factor 1 at theta index P
// ------------------------------------------------------------------------------------------------
struct RecipeTab {
    const double* coef;  // [nterms]
    const int *rowstart, *ent, *tstart, *pack, *slot;
    int P, nnz;
};

// th[0..P) = theta of draw d, th[P] = 1 (lanes of one wave; the caller orders the LDS accesses)
__device__ __forceinline__ void recipe_theta(const RecipeTab& rt, const double* __restrict__ theta, long long d, int lane, double* th) {
    if (lane <= rt.P) th[lane] = lane < rt.P ? theta[(size_t)d * rt.P + lane] : 1.0;
}

// fp[tau * 7 + e] = f[c][tau]^e, e = 0 ... 6, by repeated multiplication (one thread per tracer)
__device__ __forceinline__ void recipe_fpow(const double* __restrict__ f, int c, int ntr, int tid, double* fp) {
    if (tid < ntr) {
        const double fv = f[(size_t)c * ntr + tid];
        double p = 1.0;
        for (int e = 0; e < RECIPE_FPOW; ++e) {
            fp[tid * RECIPE_FPOW + e] = p;
            p *= fv;
        }
    }
}

// the value of entry n: its terms summed in their order
__device__ __forceinline__ double recipe_entry(const RecipeTab& rt, int n, const double* fp, const double* th) {
    double s = 0.0;
    for (int t = rt.tstart[n]; t < rt.tstart[n + 1]; ++t) {
        const int p = rt.pack[t];
        s += rt.coef[t] * fp[p >> 18] * th[p & 63] * th[(p >> 6) & 63] * th[(p >> 12) & 63];
    }
    return s;
}

// column of W_c / R^ an entry (tau * 32 + r) acts on: (tau, r) for the 24 template rows, the NNLO columns after them
__device__ __forceinline__ int recipe_col(int ent, int ntr) {
    const int tau = ent >> 5, r = ent & 31;
    return r < NROW ? tau * NROW + r : ntr * NROW + 3 * tau + (r - NROW);
}

// The forward pass of a params draw up to G (one wave; th, val, Hs and Gs are the wave's LDS, Ws, fp and col the workgroup's): theta,
// val[n], H = R^ W_c and G = H R^^T as described at draws_logp_params_kernel.  G is ordered for the wave's reads on return.
// WHO changes nothing in the function: the drag kernel instantiates its own copy (WHO = 1), because a sixth caller of the copy that the
// five params kernels share moved their compiled code by a register or two; the HMC kernel likewise (WHO = 2).
template <bool TWO, int WHO = 0>
__device__ __forceinline__ void draws_recipe_forward(const RecipeTab& rt, const double* __restrict__ theta, long long d, int lane, int ng1, int J1,
                                                     const double* Ws, const double* fp, const int* col, double* th, double* val, double* Hs, double* Gs) {
    const int J = J1 - 1, nnz = rt.nnz;
    const bool c0 = lane < J1, c1 = TWO && lane + 64 < J1;
    // ---- the non-zeros of R^ for this draw
    recipe_theta(rt, theta, d, lane, th);
    wave_lds_sync();
    for (int n = lane; n < nnz; n += 64) val[n] = recipe_entry(rt, n, fp, th);
    wave_lds_sync();
    // ---- H = R^ W_c
    for (int g = 0; g < ng1; ++g) {
        double h0 = 0.0, h1 = 0.0;
        const int n1 = rt.rowstart[g + 1];
        for (int n = rt.rowstart[g]; n < n1; ++n) {
            const double rv = val[n];
            const double* wk = Ws + col[n] * J1 + lane;
            h0 = fma(rv, c0 ? wk[0] : 0.0, h0);
            if (TWO) h1 = fma(rv, c1 ? wk[64] : 0.0, h1);
        }
        if (g == 0) {  // the data row: R^[0][J] = 1
            h0 += c0 ? Ws[J * J1 + lane] : 0.0;
            if (TWO) h1 += c1 ? Ws[J * J1 + 64 + lane] : 0.0;
        }
        if (c0) Hs[g * J1 + lane] = h0;
        if (c1) Hs[g * J1 + 64 + lane] = h1;
    }
    wave_lds_sync();
    // ---- G = H R^^T over the non-zeros of row h
    {
        const int g = lane & 31, half = lane >> 5;
        const double* hg = Hs + (g < ng1 ? g : 0) * J1;
        for (int h = 0; h < ng1; ++h) {
            double acc = 0.0;
            const int n1 = rt.rowstart[h + 1];
            for (int n = rt.rowstart[h] + half; n < n1; n += 2) acc = fma(hg[col[n]], val[n], acc);
            acc += __shfl_xor(acc, 32);
            if (h == 0) acc += hg[J];
            if (half == 0 && g < ng1) Gs[g * ng1 + h] = acc;
        }
    }
    wave_lds_sync();
}

// What a params draw kernel of one kind does between its early exit and its first draw: W_c of walker c, col[n] (the column of entry n) and,
// where the kind has them, erow[n] (its row), drow | dcol (row and column of every derivative record) and the prior table, then the powers
// of f, go to the workgroup's LDS at the places of L.  Behind the barrier: the start of wave wv's part.  (The pointers themselves are the
// kernel's, sm + L.x and the wave's start + L.x: handed back in a struct they cost every kernel some twenty registers.)
template <DrawKind KIND>
__device__ __forceinline__ double* draws_stage(const DrawLds& L, double* sm, int wv, int c, int ntr, int J1, const RecipeTab& rt,
                                               const double* __restrict__ f, const double* __restrict__ W,
                                               const int* __restrict__ erow_tab = nullptr, const int* __restrict__ dent = nullptr, int ndt = 0,
                                               const double* __restrict__ prior = nullptr) {
    int *col = reinterpret_cast<int*>(sm + L.col), *erow = reinterpret_cast<int*>(sm + L.erow);
    for (int e = threadIdx.x; e < J1 * J1; e += blockDim.x) sm[e] = W[(size_t)c * J1 * J1 + e];
    for (int n = threadIdx.x; n < rt.nnz; n += blockDim.x) {
        col[n] = recipe_col(rt.ent[n], ntr);
        if (DrawLds::has_erow(KIND)) erow[n] = erow_tab[n];
    }
    if (KIND == DRAW_HESS) {
        int *drow = reinterpret_cast<int*>(sm + L.drow), *dcol = reinterpret_cast<int*>(sm + L.dcol);
        for (int t = threadIdx.x; t < ndt; t += blockDim.x) {
            const int n = dent[t];
            drow[t] = erow_tab[n];
            dcol[t] = recipe_col(rt.ent[n], ntr);
        }
    }
    if (KIND == DRAW_CHAIN || KIND == DRAW_HMC)
        for (int e = threadIdx.x; e < CHAIN_PRI; e += blockDim.x) sm[L.pr + e] = prior[e];
    recipe_fpow(f, c, ntr, threadIdx.x, sm + L.fp);
    __syncthreads();
    return sm + L.wg + wv * L.wave;
}

// draws_logp_kernel for draws given as theta [N][P] and f [C][ntr]: the same workgroup shape (W_c in LDS once, one wave per draw at a
// time) and the same algebra after G (draws_solve), but R^ only exists as the values of its nnz non-zero entries in the wave's LDS:
//   val[n]        lanes over the entries of the recipe
//   H = R^ W_c    row g at a time: lanes over the columns j (j = lane and lane + 64 with TWO), one FMA per non-zero of row g, the value a
//                 broadcast LDS read; R^[0][J] = 1 stays implicit (the data row of W_c is added to row 0)
//   G = H R^^T    lane g + 32 half holds row g of H and takes every second non-zero of row h; the halves are added with one shuffle
// LDS: DrawLds, DRAW_PARAMS.
template <bool TWO>
__global__ __launch_bounds__(256) void draws_logp_params_kernel(int ntr, int nG, int J1, int jeffreys, RecipeTab rt, const long long* __restrict__ offsets,
                                                                const double* __restrict__ theta, const double* __restrict__ f,
                                                                const double* __restrict__ W, const double* __restrict__ mu,
                                                                const double* __restrict__ sinv, double* __restrict__ out) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng1 = nG + 1;
    const long long d0 = offsets[c], d1 = offsets[c + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;  // (workgroup-uniform: no draw for this share)
    const DrawLds L(DRAW_PARAMS, J1, nG, rt.nnz, 0, rt.P, jeffreys);
    double* wave = draws_stage<DRAW_PARAMS>(L, sm, wv, c, ntr, J1, rt, f, W);
    double *Ws = sm, *fp = sm + L.fp, *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G;
    const int* col = reinterpret_cast<int*>(sm + L.col);
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        draws_recipe_forward<TWO>(rt, theta, d, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
        draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, out + (size_t)d * MARG_OUT);
        wave_lds_sync();  // (the next draw overwrites th, val, H and G)
    }
}

// The bias recipe of eftb_draws_reduce_params evaluated into the coefficient buffers of draws_reduce_kernel: bias [N][ntr][24] and, with
// NNLO, biasn [N][ntr][3] (zero where the recipe has no entry: every coefficient is written once).  One workgroup per (walker, share of its draws), one wave per draw at a time.
// LDS: fp [RECIPE_MAXTR * 7], then per wave th [34].
template <bool NNLO>
__global__ __launch_bounds__(256) void draws_recipe_rows_kernel(int ntr, RecipeTab rt, const long long* __restrict__ offsets, const double* __restrict__ theta,
                                                                const double* __restrict__ f, double* __restrict__ bias, double* __restrict__ biasn) {
    __shared__ double fp[RECIPE_MAXTR * RECIPE_FPOW];
    __shared__ double ths[4][34];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long d0 = offsets[c], d1 = offsets[c + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;
    recipe_fpow(f, c, ntr, threadIdx.x, fp);
    __syncthreads();
    double* th = ths[wv];
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        recipe_theta(rt, theta, d, lane, th);
        wave_lds_sync();
        for (int q = lane; q < ntr * (NROW + 3); q += 64) {
            const int tau = q / (NROW + 3), r = q % (NROW + 3), n = rt.slot[q];
            const double v = n >= 0 ? recipe_entry(rt, n, fp, th) : 0.0;
            if (r < NROW) bias[((size_t)d * ntr + tau) * NROW + r] = v;
            else if (NNLO) biasn[((size_t)d * ntr + tau) * 3 + (r - NROW)] = v;
        }
        wave_lds_sync();  // (the next draw overwrites th)
    }
}

// ------------------------------------------------------------------------------------------------
// d ln P / d theta of a params draw by an adjoint pass (eftb_draws_logp_grad_params).  With v = (1, b):
//     d chi2 = sum_gh S[g][h] dG[g][h],   S = v v^T + [not Jeffreys] blockdiag(0, F2^-1),   dG = dR^ W_c R^^T + R^ W_c dR^^T
//     Rbar = d chi2 / d R^ = (S + S^T) H    (needed at the nnz entries of the recipe only),    d ln P / d theta_p = -1/2 sum_n Rbar[n] d val[n] / d theta_p
// The derivative of the recipe is a second table built by eftb_set_draw_recipe (kind 0) from the sorted terms, one record per (term, distinct
// theta index p in it), sorted by (p, entry, parent term):
//   dtab = pstart [P + 1] (first record of parameter p) | dent [ndt] (the entry n the record belongs to) | dpack [ndt] | erow [nnz] (row g of entry n)
//   dpack = i | j << 6 | (tau * 7 + e) << 18: the two remaining theta indices (the factor 1 at index P); dcoef = coef * multiplicity of p
// ------------------------------------------------------------------------------------------------
struct RecipeGradTab {
    const double* dcoef;  // [ndt]
    const int *pstart, *dent, *dpack, *erow;
    int lgP2;  // log2 of the smallest power of two >= max(P, 1): lane = share << lgP2 | p in the P sums
};

// The adjoint of one draw behind draws_solve<true> (S over G, ordered for the wave's reads): Rbar over val, then the P sums and their
// butterfly -> sum_n Rbar[n] d val[n] / d theta_p in every lane whose low bits are p (-2 d ln P / d theta_p).  The gradient kernel and
// the HMC kernel both call it, so a gradient has the same bits whichever call computed it.
__device__ __forceinline__ double draws_grad_adjoint(const RecipeGradTab& gt, int lane, int ng1, int J1, int nnz, int P, const double* fp, const int* col,
                                                     const int* erow, const double* th, double* val, const double* Hs, const double* Gs) {
    const int pmask = (1 << gt.lgP2) - 1, gp = lane & pmask, share = lane >> gt.lgP2, nshare = 64 >> gt.lgP2;
    // ---- Rbar at the non-zeros, over val
    for (int n = lane; n < nnz; n += 64) {
        const int g = erow[n];
        const double* hc = Hs + col[n];
        double acc = 0.0;
        for (int h = 0; h < ng1; ++h) acc = fma(Gs[g * ng1 + h] + Gs[h * ng1 + g], hc[h * J1], acc);
        val[n] = acc;
    }
    wave_lds_sync();
    // ---- the P sums over the derivative table
    double acc = 0.0;
    if (gp < P) {
        const int t1 = gt.pstart[gp + 1];
        for (int t = gt.pstart[gp] + share; t < t1; t += nshare) {
            const int q = gt.dpack[t];
            acc = fma(gt.dcoef[t] * fp[q >> 18] * th[q & 63] * th[(q >> 6) & 63], val[gt.dent[t]], acc);
        }
    }
    for (int m = 32; m > pmask; m >>= 1) acc += __shfl_xor(acc, m);
    return acc;
}

// draws_logp_params_kernel with the gradient: the same outer shape and forward pass (draws_recipe_forward), then per draw
//   solve          draws_solve<true>: the record, and S over G
//   Rbar[n]        lanes over the entries n = (g, col): sum_h (S[g][h] + S[h][g]) H[h][col], written over val[n] (the computed F2^-1 is
//                  symmetric up to rounding only: both halves of dG get their own factor)
//   grad[p]        lane = share << lgP2 | p: share s of the 64 >> lgP2 takes every (64 >> lgP2)-th record of parameter p in table order,
//                  the shares are added by an xor butterfly over the share bits (a fixed tree: the same bits however the grid is split)
// A draw with det F2 <= 0 gets NaN in all P slots.  LDS: DrawLds, DRAW_GRAD.
template <bool TWO>
__global__ __launch_bounds__(256) void draws_logp_grad_params_kernel(int ntr, int nG, int J1, int jeffreys, RecipeTab rt, RecipeGradTab gt,
                                                                     const long long* __restrict__ offsets, const double* __restrict__ theta,
                                                                     const double* __restrict__ f, const double* __restrict__ W,
                                                                     const double* __restrict__ mu, const double* __restrict__ sinv,
                                                                     double* __restrict__ out, double* __restrict__ grad) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng1 = nG + 1, nnz = rt.nnz, P = rt.P;
    const long long d0 = offsets[c], d1 = offsets[c + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;  // (workgroup-uniform: no draw for this share)
    const DrawLds L(DRAW_GRAD, J1, nG, nnz, 0, P, jeffreys);
    double* wave = draws_stage<DRAW_GRAD>(L, sm, wv, c, ntr, J1, rt, f, W, gt.erow);
    double *Ws = sm, *fp = sm + L.fp, *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G;
    const int *col = reinterpret_cast<int*>(sm + L.col), *erow = reinterpret_cast<int*>(sm + L.erow);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        draws_recipe_forward<TWO>(rt, theta, d, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
        const bool ok = draws_solve<true>(lane, nG, jeffreys, Gs, mu, sinv, out + (size_t)d * MARG_OUT);
        wave_lds_sync();
        const double acc = draws_grad_adjoint(gt, lane, ng1, J1, nnz, P, fp, col, erow, th, val, Hs, Gs);
        if (lane < P) grad[(size_t)d * P + lane] = ok ? -0.5 * acc : nan;
        wave_lds_sync();  // (the next draw overwrites th, val, H and G)
    }
}

// ------------------------------------------------------------------------------------------------
// d2 ln P / d theta d theta of a params draw (eftb_draws_logp_hess_params).  With K = F2^-1, D_p = d R^ / d theta_p (the derivative records
// of p: value dval, row g, column c), G_p = D_p H^T + H D_p^T and u_p = (G_p v)[1:]:
//     d2 chi2 / d theta_p d theta_q = sum_n Rbar[n] d2 val_n / d theta_p d theta_q                                (t1: the second-derivative records)
//                                   + sum_{n of p, m of q} dval_n dval_m (S + S^T)[g_n][g_m] W_c[c_n][c_m]        (t2)
//                                   - 2 u_p^T K u_q  -  [not Jeffreys] sum_ij M_p[i][j] M_q[j][i],  M_p = K G_p[1:,1:]   (t3, t4)
// and d2 ln P = -1/2 of that.  The second-derivative table of eftb_set_draw_recipe (kind 0), one record per (term, pair p <= q of theta
// indices in it), sorted by (p, q, entry, parent term):
//   htab = hstart [P (P + 1) / 2 + 1] (first record of pair (p, q), pairs in row order of the upper triangle) | hent [nh] | hpack [nh]
//   hpack = i | (tau * 7 + e) << 18: the one remaining theta index (the factor 1 at index P); hcoef = coef * multiplicity
// ------------------------------------------------------------------------------------------------
struct RecipeHessTab {
    const double* hcoef;  // [nh]
    const int *hstart, *hent, *hpack;
    int ndt, npair, lgPP;  // derivative records; pairs; log2 of the smallest power of two >= min(npair, 64): lane = share << lgPP | pair
};

// draws_logp_grad_params_kernel with the Hessian: the same forward pass, solve (draws_solve<true, true>: K also under Jeffreys, kept beside
// S), Rbar and gradient sums, so the record and the gradient are the gradient call's bits.  Then per draw
//   dval[t], hv    lanes over the derivative records: their values; lanes over the columns: hv = H^T v
//   u_p, G_p       lanes over (p, i) and (p, i, j): the records of p in table order against H and hv
//   w_q, M_p       lanes over (q, i) and (p, i, j): K u_q and K G_p[1:,1:]
//   hess[p][q]     lane = share << lgPP | pair (64 pairs at a time): share s takes every (64 >> lgPP)-th second-derivative record (t1),
//                  derivative record of p (t2, against every record of q), i (t3) and (i, j) (t4) of its pair; the shares are added by
//                  an xor butterfly over the share bits.  Assignment and tree depend on the recipe alone.
// Entry (q, p) is a copy of (p, q).  A draw with det F2 <= 0 gets NaN in all P^2 slots, as in grad and ln P.  Every loop is bounded by a
// table size.  LDS: DrawLds, DRAW_HESS.
template <bool TWO>
__global__ __launch_bounds__(256) void draws_logp_hess_params_kernel(int ntr, int nG, int J1, int jeffreys, RecipeTab rt, RecipeGradTab gt, RecipeHessTab ht,
                                                                     const long long* __restrict__ offsets, const double* __restrict__ theta,
                                                                     const double* __restrict__ f, const double* __restrict__ W,
                                                                     const double* __restrict__ mu, const double* __restrict__ sinv,
                                                                     double* __restrict__ out, double* __restrict__ grad, double* __restrict__ hess) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng1 = nG + 1, nnz = rt.nnz, P = rt.P, ndt = ht.ndt, nG2 = nG * nG;
    const long long d0 = offsets[c], d1 = offsets[c + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;  // (workgroup-uniform: no draw for this share)
    const DrawLds L(DRAW_HESS, J1, nG, nnz, ndt, P, jeffreys);
    double* wave = draws_stage<DRAW_HESS>(L, sm, wv, c, ntr, J1, rt, f, W, gt.erow, gt.dent, ndt);
    double *Ws = sm, *fp = sm + L.fp, *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G;
    double *Ks = wave + L.K, *dval = wave + L.dval, *hv = wave + L.hv, *us = wave + L.u, *ws = wave + L.w, *Gp = wave + L.Gp, *Mp = wave + L.Mp;
    const int *col = reinterpret_cast<int*>(sm + L.col), *erow = reinterpret_cast<int*>(sm + L.erow);
    const int *drow = reinterpret_cast<int*>(sm + L.drow), *dcol = reinterpret_cast<int*>(sm + L.dcol);
    const int gpn = jeffreys ? 0 : P * nG2;
    const int pmask = (1 << gt.lgP2) - 1, gp = lane & pmask, share = lane >> gt.lgP2, nshare = 64 >> gt.lgP2;
    const int qmask = (1 << ht.lgPP) - 1, hshare = lane >> ht.lgPP, nhshare = 64 >> ht.lgPP;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        draws_recipe_forward<TWO>(rt, theta, d, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
        const bool ok = draws_solve<true, true>(lane, nG, jeffreys, Gs, mu, sinv, out + (size_t)d * MARG_OUT, Ks);
        wave_lds_sync();
        // ---- Rbar at the non-zeros, over val; the values of the derivative records; hv = H^T v (v[g] = S[g][0])
        for (int n = lane; n < nnz; n += 64) {
            const int g = erow[n];
            const double* hc = Hs + col[n];
            double acc = 0.0;
            for (int h = 0; h < ng1; ++h) acc = fma(Gs[g * ng1 + h] + Gs[h * ng1 + g], hc[h * J1], acc);
            val[n] = acc;
        }
        for (int t = lane; t < ndt; t += 64) {
            const int q = gt.dpack[t];
            dval[t] = gt.dcoef[t] * fp[q >> 18] * th[q & 63] * th[(q >> 6) & 63];
        }
        for (int j = lane; j < J1; j += 64) {
            double acc = 0.0;
            for (int g = 0; g < ng1; ++g) acc = fma(Gs[g * ng1], Hs[g * J1 + j], acc);
            hv[j] = acc;
        }
        wave_lds_sync();
        // ---- the P sums over the derivative table (as the gradient kernel)
        {
            double acc = 0.0;
            if (gp < P) {
                const int t1 = gt.pstart[gp + 1];
                for (int t = gt.pstart[gp] + share; t < t1; t += nshare) {
                    const int q = gt.dpack[t];
                    acc = fma(gt.dcoef[t] * fp[q >> 18] * th[q & 63] * th[(q >> 6) & 63], val[gt.dent[t]], acc);
                }
            }
            for (int m = 32; m > pmask; m >>= 1) acc += __shfl_xor(acc, m);
            if (lane < P) grad[(size_t)d * P + lane] = ok ? -0.5 * acc : nan;
        }
        // ---- u_p and G_p[1:,1:] from the records of p in table order
        for (int e = lane; e < P * nG; e += 64) {
            const int p = e / nG, g = e % nG + 1;
            const double* hg = Hs + g * J1;
            double acc = 0.0;
            const int t1 = gt.pstart[p + 1];
            for (int t = gt.pstart[p]; t < t1; ++t) {
                const int gt_ = drow[t], ct = dcol[t];
                acc = fma(dval[t], fma(Gs[gt_ * ng1], hg[ct], gt_ == g ? hv[ct] : 0.0), acc);
            }
            us[e] = acc;
        }
        for (int e = lane; e < gpn; e += 64) {
            const int p = e / nG2, r = e % nG2, i = r / nG + 1, j = r % nG + 1;
            const double *hi = Hs + i * J1, *hj = Hs + j * J1;
            double acc = 0.0;
            const int t1 = gt.pstart[p + 1];
            for (int t = gt.pstart[p]; t < t1; ++t) {
                const int gt_ = drow[t], ct = dcol[t];
                acc = fma(dval[t], (gt_ == i ? hj[ct] : 0.0) + (gt_ == j ? hi[ct] : 0.0), acc);
            }
            Gp[e] = acc;
        }
        wave_lds_sync();
        // ---- w_q = K u_q and M_p = K G_p[1:,1:]
        for (int e = lane; e < P * nG; e += 64) {
            const int q = e / nG, i = e % nG;
            double acc = 0.0;
            for (int k = 0; k < nG; ++k) acc = fma(Ks[i * nG + k], us[q * nG + k], acc);
            ws[e] = acc;
        }
        for (int e = lane; e < gpn; e += 64) {
            const int p = e / nG2, r = e % nG2, i = r / nG, j = r % nG;
            const double* gpp = Gp + p * nG2 + j;
            double acc = 0.0;
            for (int k = 0; k < nG; ++k) acc = fma(Ks[i * nG + k], gpp[k * nG], acc);
            Mp[e] = acc;
        }
        wave_lds_sync();
        // ---- the P (P + 1) / 2 sums, 64 >> lgPP shares per pair
        for (int base = 0; base < ht.npair; base += 64) {
            const int pair = base + (lane & qmask);
            double acc = 0.0;
            int p = 0, q = 0;
            if (pair < ht.npair) {
                int r = pair;
                while (p < P && r >= P - p) {  // (at most P steps)
                    r -= P - p;
                    ++p;
                }
                q = p + r;
                // t1
                const int h1 = ht.hstart[pair + 1];
                for (int t = ht.hstart[pair] + hshare; t < h1; t += nhshare) {
                    const int k = ht.hpack[t];
                    acc = fma(ht.hcoef[t] * fp[k >> 18] * th[k & 63], val[ht.hent[t]], acc);
                }
                // t2
                const int n1 = gt.pstart[p + 1], m0 = gt.pstart[q], m1 = gt.pstart[q + 1];
                for (int n = gt.pstart[p] + hshare; n < n1; n += nhshare) {
                    const int gn = drow[n];
                    const double* wn = Ws + dcol[n] * J1;
                    double s = 0.0;
                    for (int m = m0; m < m1; ++m) {
                        const int gm = drow[m];
                        s = fma(dval[m] * (Gs[gn * ng1 + gm] + Gs[gm * ng1 + gn]), wn[dcol[m]], s);
                    }
                    acc = fma(dval[n], s, acc);
                }
                // t3
                for (int i = hshare; i < nG; i += nhshare) acc = fma(-2.0 * us[p * nG + i], ws[q * nG + i], acc);
                // t4
                if (!jeffreys)
                    for (int r2 = hshare; r2 < nG2; r2 += nhshare) {
                        const int i = r2 / nG, j = r2 % nG;
                        acc = fma(-Mp[p * nG2 + i * nG + j], Mp[q * nG2 + j * nG + i], acc);
                    }
            }
            for (int m = 32; m > qmask; m >>= 1) acc += __shfl_xor(acc, m);
            if (hshare == 0 && pair < ht.npair) {
                const double hv2 = ok ? -0.5 * acc : nan;
                hess[((size_t)d * P + p) * P + q] = hv2;
                hess[((size_t)d * P + q) * P + p] = hv2;
            }
        }
        wave_lds_sync();  // (the next draw overwrites th, val, H, G and the Hessian's scratch)
    }
}

// ------------------------------------------------------------------------------------------------
// Draw calls against many data vectors sharing one covariance (eftb_draws_logp_params_datasets).  Only the last row and column of W_c depend
// on the data: a group g = (walker c, data set m) gets
//     Wg[g][:J][:J] = W_c[:J][:J],     Wg[g][i][J] = Wg[g][J][i] = (A_i . U_J + A_J . U_i) / 2,     A_J = -d_m,  U_J = -(d_m C^-1)
// with A_c, U_c = A_c C^-1 and W_c of draws_gram and D [M][ndata], Ud = D C^-1 of eftb_set_likelihood_datasets.  One workgroup per group.  The
// border sums are those of draws_gram_kernel for the entries (i, J), i <= J: one 16-lane group per entry, lanes stride the data index, the FMA
// chains s0 and s1, the same xor tree; the negations are exact, so a data set equal to the likelihood's own vector gives the bits of W_c.
// ------------------------------------------------------------------------------------------------
template <int NT>  // threads per workgroup, a multiple of 16
__global__ __launch_bounds__(NT) void draws_gram_groups_kernel(int ndata, int J1, const int* __restrict__ walker, const int* __restrict__ dataset,
                                                                const double* __restrict__ A, const double* __restrict__ U,
                                                                const double* __restrict__ W, const double* __restrict__ D,
                                                                const double* __restrict__ Ud, double* __restrict__ Wg) {
    const int g = blockIdx.x, sub = threadIdx.x & 15, grp = threadIdx.x >> 4, J = J1 - 1;
    const int c = walker[g], m = dataset[g];
    const double* Ac = A + (size_t)c * J1 * ndata;
    const double* Uc = U + (size_t)c * J1 * ndata;
    const double* Wc = W + (size_t)c * J1 * J1;
    const double* dm = D + (size_t)m * ndata;
    const double* um = Ud + (size_t)m * ndata;
    double* Wo = Wg + (size_t)g * J1 * J1;
    for (int e = threadIdx.x; e < J1 * J1; e += NT)
        if (e / J1 < J && e % J1 < J) Wo[e] = Wc[e];
    for (int i = grp; i < J1; i += NT / 16) {  // entry (i, J); i is uniform over the 16-lane group: the shuffles stay inside it
        double s0 = 0.0, s1 = 0.0;
        for (int b = sub; b < ndata; b += 16) {
            const double aJ = -dm[b], uJ = -um[b];
            s0 = fma(i < J ? Ac[(size_t)i * ndata + b] : aJ, uJ, s0);
            s1 = fma(aJ, i < J ? Uc[(size_t)i * ndata + b] : uJ, s1);
        }
#pragma unroll
        for (int q = 8; q >= 1; q >>= 1) {
            s0 += __shfl_xor(s0, q, 16);
            s1 += __shfl_xor(s1, q, 16);
        }
        if (sub == 0) {
            const double w = 0.5 * (s0 + s1);
            Wo[(size_t)i * J1 + J] = w;
            Wo[(size_t)J * J1 + i] = w;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Samples of the marginalised parameters of a params draw (eftb_draws_sample_params).  Given theta they are exactly Gaussian,
//     b | theta, data ~ N(b^ = F2^-1 F1, F2^-1)      (with and without Jeffreys, which only drops ln det F2 from the marginal),
// so with the upper Cholesky factor F2 = U^T U and standard normals z of the caller, b = b^ + U^-1 z has that law: cov(U^-1 z) = U^-1 U^-T.
// draws_logp_params_kernel's outer shape and forward pass (draws_recipe_forward), then per draw
//   record         draws_solve<false>: the same function, so ln P, full chi2 and b^ are the bits of eftb_draws_logp_params; G stays in the LDS
//   Cholesky       wave-synchronous, on F2 as draws_solve's first statement forms it: lane i < nG keeps row i in registers, no pivot search
//                  and no row exchange.  Column c: the pivot a_c[c] is broadcast from lane c, r = sqrt(pivot); the rows i > c eliminate
//                  with m = a_i[c] / pivot, a_i[j] = fma(-m, a_c[j], a_i[j]) (j > c); row c becomes U[c][j] = a_c[j] / r (j >= c).
//                  A pivot that is not > 0 (NaN included) marks the draw failed, wave-uniformly
//   samples        ADJ_KB at a time, independent chains as the F2^-1 columns of draws_solve<true>: lane i starts with y = z[d][s][i];
//                  for c = nG - 1 ... 0: x_c = y of lane c / U[c][c], lanes i < c take y = fma(-U[i][c], x_c, y); b[s][i] = b^[i] + x_i.
//                  The chains never mix: a sample's bits depend neither on S, nor on its place in the chunk, the split into calls or the wave
//   chi2(b[s])     draws_solve's `full` formula G[0][0] + 2 b . G[1:,0] + b^T G[1:,1:] b in the same row order (z = 0: the bits of the record's)
//   coefficients   (coef != null) coef[d][s][tau][r] = R^[0][(tau, r)] + sum_g b[s][g - 1] R^[g][(tau, r)] over the entries val[n] of the recipe
//                  in table order: lanes over the 27 ntr slots, zero where the recipe has no entry, every coefficient written once (as
//                  draws_recipe_rows_kernel); the 24 template coefficients to coef [N S][ntr][24], the NNLO ones to coefn [N S][ntr][3]
// A failed draw (det F2 <= 0 of draws_solve, or a pivot <= 0) gets NaN in all S samples, their chi2 and its coefficient rows; its record is
// what draws_solve wrote.  LDS: DrawLds, DRAW_SAMPLE.
// ------------------------------------------------------------------------------------------------
template <bool TWO>
__global__ __launch_bounds__(256) void draws_sample_params_kernel(int ntr, int nG, int J1, int jeffreys, int S, RecipeTab rt, const int* __restrict__ erow_tab,
                                                                  const long long* __restrict__ offsets, const double* __restrict__ theta,
                                                                  const double* __restrict__ f, const double* __restrict__ W,
                                                                  const double* __restrict__ mu, const double* __restrict__ sinv,
                                                                  const double* __restrict__ z, double* __restrict__ out, double* __restrict__ bsamp,
                                                                  double* __restrict__ chi2samp, double* __restrict__ coef, double* __restrict__ coefn) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng1 = nG + 1, nnz = rt.nnz;
    const long long d0 = offsets[c], d1 = offsets[c + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;  // (workgroup-uniform: no draw for this share)
    const DrawLds L(DRAW_SAMPLE, J1, nG, nnz, 0, rt.P, jeffreys);
    double* wave = draws_stage<DRAW_SAMPLE>(L, sm, wv, c, ntr, J1, rt, f, W, erow_tab);
    double *Ws = sm, *fp = sm + L.fp, *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G, *bs = wave + L.bs;
    const int *col = reinterpret_cast<int*>(sm + L.col), *erow = reinterpret_cast<int*>(sm + L.erow);
    const bool own = lane < nG;
    const int nslot = ntr * (NROW + 3);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        double* o = out + (size_t)d * MARG_OUT;
        draws_recipe_forward<TWO>(rt, theta, d, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
        bool good = draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, o);
        // ---- F2 = U^T U: lane i ends with row i of U
        double a[MARG_MAXG], dg[MARG_MAXG];
#pragma unroll
        for (int j = 0; j < MARG_MAXG; ++j)
            a[j] = (own && j < nG) ? 0.5 * (Gs[(lane + 1) * ng1 + j + 1] + Gs[(j + 1) * ng1 + lane + 1]) + (lane == j ? sinv[j] : 0.0) : 0.0;
#pragma unroll
        for (int c2 = 0; c2 < MARG_MAXG; ++c2) {
            dg[c2] = 1.0;
            if (c2 < nG) {
                const double piv = readlane_f64(a[c2], c2);
                if (!(piv > 0.0)) good = false;
                const double r = sqrt(piv);
                const bool elim = own && lane > c2;
                const double m = elim ? a[c2] / piv : 0.0;
#pragma unroll
                for (int j = c2; j < MARG_MAXG; ++j)
                    if (j < nG) {
                        const double u = readlane_f64(a[j], c2);
                        if (elim && j > c2) a[j] = fma(-m, u, a[j]);
                        if (lane == c2) a[j] = u / r;
                    }
                dg[c2] = readlane_f64(a[c2], c2);  // U[c2][c2]
            }
        }
        const double bhat = own ? o[2 + lane] : 0.0;  // (this lane's own store in draws_solve)
        for (int s0 = 0; s0 < S; s0 += ADJ_KB) {
            // ---- U x = z, ADJ_KB samples at a time
            double y[ADJ_KB];
#pragma unroll
            for (int q = 0; q < ADJ_KB; ++q) y[q] = (own && s0 + q < S) ? z[((size_t)d * S + s0 + q) * nG + lane] : 0.0;
#pragma unroll
            for (int c2 = MARG_MAXG - 1; c2 >= 0; --c2)
                if (c2 < nG) {
                    const bool above = own && lane < c2;
#pragma unroll
                    for (int q = 0; q < ADJ_KB; ++q) {
                        const double xc = readlane_f64(y[q], c2) / dg[c2];
                        if (above) y[q] = fma(-a[c2], xc, y[q]);
                        if (lane == c2) y[q] = xc;
                    }
                }
            double bi[ADJ_KB];
#pragma unroll
            for (int q = 0; q < ADJ_KB; ++q) {
                bi[q] = bhat + y[q];
                if (own) {
                    bs[q * nG + lane] = bi[q];
                    if (s0 + q < S) bsamp[((size_t)d * S + s0 + q) * nG + lane] = good ? bi[q] : nan;
                }
            }
            wave_lds_sync();
            // ---- chi2 at b[s] (row sums per lane, added in row order, as draws_solve)
#pragma unroll
            for (int q = 0; q < ADJ_KB; ++q) {
                double srow = 0.0;
#pragma unroll
                for (int j = 0; j < MARG_MAXG; ++j)
                    if (j < nG && own) srow = fma(bs[q * nG + j], Gs[(lane + 1) * ng1 + j + 1], srow);
                const double trow = own ? bi[q] * fma(2.0, Gs[(lane + 1) * ng1], srow) : 0.0;
                double full = Gs[0];
#pragma unroll
                for (int i = 0; i < MARG_MAXG; ++i)
                    if (i < nG) full += readlane_f64(trow, i);
                if (lane == 0 && s0 + q < S) chi2samp[(size_t)d * S + s0 + q] = good ? full : nan;
            }
            // ---- the coefficient rows of the samples: lanes over the slots (tau, r), the entries of the recipe in table order
            if (coef) {
                for (int q0 = 0; q0 < nslot; q0 += 64) {
                    const int sl = q0 + lane, tau = sl / (NROW + 3), r = sl % (NROW + 3);
                    const int cq = sl < nslot ? recipe_col(tau * 32 + r, ntr) : -1;
                    double acc[ADJ_KB];
#pragma unroll
                    for (int q = 0; q < ADJ_KB; ++q) acc[q] = 0.0;
                    for (int n = 0; n < nnz; ++n) {
                        const int g = erow[n];
                        const double v = val[n];
                        const bool mine = col[n] == cq;
#pragma unroll
                        for (int q = 0; q < ADJ_KB; ++q) {
                            const double bg = g ? bs[q * nG + g - 1] : 1.0;
                            if (mine) acc[q] = fma(bg, v, acc[q]);
                        }
                    }
                    if (sl < nslot) {
#pragma unroll
                        for (int q = 0; q < ADJ_KB; ++q)
                            if (s0 + q < S) {
                                const size_t row = ((size_t)d * S + s0 + q) * ntr + tau;
                                if (r < NROW) coef[row * NROW + r] = good ? acc[q] : nan;
                                else if (coefn) coefn[row * 3 + (r - NROW)] = good ? acc[q] : nan;
                            }
                    }
                }
            }
            wave_lds_sync();  // (the next chunk overwrites bs)
        }
        wave_lds_sync();  // (the next draw overwrites th, val, H and G)
    }
}

// ------------------------------------------------------------------------------------------------
// Metropolis chains over theta at fixed templates (eftb_draws_chain_params): one wave per chain, all steps of a launch in the kernel.
// Target ln pi(theta) = ln P_marg(theta) + pri(theta), pri = -1/2 sum_p ((theta_p - loc_p) sinv_p)^2 inside the box [lower, upper].
// Nothing random happens here: the caller supplies the increments step [N][Tc][P] and lnu [N][Tc] = ln of its uniforms.
// draws_logp_params_kernel's outer shape and staging, then per chain
//   start          the record of the starting theta (draws_recipe_forward + draws_solve<false>: the bits of eftb_draws_logp_params), its pri;
//                  ln P not finite there (det F2 <= 0 gives NaN), or an accept count of -1 from an earlier launch: the chain has failed,
//                  NaN in its slots and in theta, accept count -1
//   step i         theta' = theta + step[i]; outside the box: rejected without an evaluation.  Otherwise the forward pass and solve at
//                  theta' into the record slot that is not the current one, then
//                      accept iff ln P' is finite and lnu[i] < (ln P' + pri') - (ln P + pri)
//                  taken from lane 0 and broadcast: the branch around the forward pass and the flip of the slot index are wave-uniform
//   store          after every thin-th step of the whole chain (t0 steps came before this launch): theta to chain [N][kstride][P], the
//                  current record to rec [N][kstride][MARG_OUT], the launch's slots 0 ... kc - 1 in turn
//   end            theta [N][P] and nacc [N] are overwritten with the state after the launch's last step: all that the next launch needs
// pri and the accept expression are evaluated with every operation rounded on its own (no contraction), in parameter order, so that
// NumPy reproduces them bit for bit; sinv_p = 0 skips parameter p.  Every loop's trip count is fixed at launch.
// LDS: DrawLds, DRAW_CHAIN; pr [4][RECIPE_MAXP] = lower | upper | loc | sinv.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double chain_prior(int P, const double* t, const double* pr) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int p = 0; p < P; ++p) {
        const double s = pr[3 * RECIPE_MAXP + p];
        if (s != 0.0) {
            const double q = (t[p] - pr[2 * RECIPE_MAXP + p]) * s;
            acc = acc + q * q;
        }
    }
    return -0.5 * acc;
}

__device__ __forceinline__ bool chain_accept(double lnu, double lp1, double pri1, double lp0, double pri0) {
#pragma clang fp contract(off)
    return __builtin_isfinite(lp1) && lnu < (lp1 + pri1) - (lp0 + pri0);
}

template <bool TWO>
__global__ __launch_bounds__(256) void draws_chain_params_kernel(int ntr, int nG, int J1, int jeffreys, int Tc, int t0, int thin, int kc, int kstride,
                                                                 RecipeTab rt, const long long* __restrict__ offsets, double* __restrict__ theta,
                                                                 long long* __restrict__ nacc, const double* __restrict__ f, const double* __restrict__ W,
                                                                 const double* __restrict__ mu, const double* __restrict__ sinv,
                                                                 const double* __restrict__ prior, const double* __restrict__ step,
                                                                 const double* __restrict__ lnu, double* __restrict__ chain, double* __restrict__ rec) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng1 = nG + 1, P = rt.P;
    const long long d0 = offsets[c], d1 = offsets[c + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;  // (workgroup-uniform: no chain for this share)
    const DrawLds L(DRAW_CHAIN, J1, nG, rt.nnz, 0, P, jeffreys);
    double* wave = draws_stage<DRAW_CHAIN>(L, sm, wv, c, ntr, J1, rt, f, W, nullptr, nullptr, 0, prior);
    double *Ws = sm, *fp = sm + L.fp, *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G;
    double *tc = wave + L.tc, *tp = wave + L.tp, *rs = wave + L.rs;
    const int* col = reinterpret_cast<int*>(sm + L.col);
    const double* pr = sm + L.pr;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        long long na = nacc[d];
        double* oc = chain + (size_t)d * kstride * P;
        double* orec = rec + (size_t)d * kstride * MARG_OUT;
        if (lane < P) tc[lane] = tp[lane] = theta[(size_t)d * P + lane];
        wave_lds_sync();
        int cur = 0;
        double lp0 = nan, pri0 = 0.0;
        if (na >= 0) {  // (wave-uniform)
            draws_recipe_forward<TWO>(rt, tp, 0, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
            draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, rs);
            wave_lds_sync();
            lp0 = rs[0];
            pri0 = chain_prior(P, tp, pr);
        }
        if (!__builtin_amdgcn_readfirstlane((int)__builtin_isfinite(lp0))) {  // a failed chain
            for (int k = 0; k < kc; ++k) {
                if (lane < P) oc[(size_t)k * P + lane] = nan;
                if (lane < MARG_OUT) orec[(size_t)k * MARG_OUT + lane] = nan;
            }
            if (lane < P) theta[(size_t)d * P + lane] = nan;
            if (lane == 0) nacc[d] = -1;
            wave_lds_sync();
            continue;
        }
        int left = thin - t0 % thin, k = 0;
        for (int i = 0; i < Tc; ++i) {
            if (lane < P) tp[lane] = tc[lane] + step[((size_t)d * Tc + i) * P + lane];
            wave_lds_sync();
            bool in = true;
            for (int p = 0; p < P; ++p) {
                const double v = tp[p];
                in = in && v >= pr[p] && v <= pr[RECIPE_MAXP + p];
            }
            int acc = 0;
            double lp1 = nan, pri1 = 0.0;
            if (__builtin_amdgcn_readfirstlane((int)in)) {  // (wave-uniform: the forward pass and the solve are wave-synchronous)
                double* ot = rs + (cur ^ 1) * MARG_OUT;
                draws_recipe_forward<TWO>(rt, tp, 0, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
                draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, ot);
                wave_lds_sync();
                lp1 = ot[0];
                pri1 = chain_prior(P, tp, pr);
                acc = __builtin_amdgcn_readfirstlane((int)chain_accept(lnu[(size_t)d * Tc + i], lp1, pri1, lp0, pri0));
            }
            if (acc) {
                cur ^= 1;
                lp0 = lp1;
                pri0 = pri1;
                ++na;
                if (lane < P) tc[lane] = tp[lane];
            }
            if (--left == 0) {
                left = thin;
                if (k < kc) {  // (always: the host counts the slots of the launch the same way)
                    if (lane < P) oc[(size_t)k * P + lane] = tc[lane];
                    if (lane < MARG_OUT) orec[(size_t)k * MARG_OUT + lane] = rs[cur * MARG_OUT + lane];
                }
                ++k;
            }
            wave_lds_sync();  // (the next step overwrites the trial theta, th, val, H, G and the other record)
        }
        if (lane < P) theta[(size_t)d * P + lane] = tc[lane];
        if (lane == 0) nacc[d] = na;
        wave_lds_sync();
    }
}

// ------------------------------------------------------------------------------------------------
// Dragging chains between two walkers (eftb_draws_drag_params): the chain kernel against a target that slides from the start walker a of
// the chain's pair to its end walker b,
//     ln pi_t(theta) = (1 - lam_t) ln pi_a(theta) + lam_t ln pi_b(theta),     ln pi_x = ln P_x + pri,     lam_t = frac[t] from the caller.
// One workgroup per (pair, share of its chains) with W_a, W_b and the powers of f_a, f_b staged once; one wave per chain at a time, the
// chain kernel's loop with two evaluations per point: draws_recipe_forward + draws_solve<false> against a, then (where ln P_a is finite:
// wave-uniform) against b, through the same th / val / H / G scratch -- every record is eftb_draws_logp_params' for that (walker, theta).
//   start          both records of the starting theta and its pri; either ln P not finite, or an accept count of -1 from an earlier launch:
//                  the chain has failed, NaN in its slots, theta, sums and final records, accept count -1.  The first launch (t0 = 0)
//                  starts the sums at sa = ln P_a + pri, sb = ln P_b + pri; a later one takes them from sums [N][2]
//   step i         as the chain kernel's, with drag_accept; the trial pair of records goes beside the current pair and the pair index
//                  flips on acceptance.  After the decision sa = sa + (ln P_a + pri), sb = sb + (ln P_b + pri) of the current state
//   store          after every thin-th step (thin = 0: never): theta and the current pair of records, rec [N][kstride][2][MARG_OUT]
//   end            theta, nacc, sums and the current pair of records (fin [N][2][MARG_OUT]) are overwritten with the state after the launch
// drag_accept and drag_sum round every operation on its own, as chain_prior and chain_accept.  Every loop's trip count is fixed at launch.
// LDS: DrawLds, DRAW_DRAG.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool drag_accept(double lnu, double lam, double la1, double lb1, double pri1, double la0, double lb0, double pri0) {
#pragma clang fp contract(off)
    const double u = 1.0 - lam;
    const double a1 = la1 + pri1, b1 = lb1 + pri1, a0 = la0 + pri0, b0 = lb0 + pri0;
    const double w1 = u * a1 + lam * b1, w0 = u * a0 + lam * b0;
    return __builtin_isfinite(la1) && __builtin_isfinite(lb1) && lnu < w1 - w0;
}

__device__ __forceinline__ double drag_sum(double s, double lp, double pri) {
#pragma clang fp contract(off)
    return s + (lp + pri);
}

// draws_stage for a pair of walkers: the end walker's W_c and powers of f go in first, then everything the chain kernel stages for the
// start walker (draws_stage of the chain kind, unchanged, at the places of the drag layout), behind one barrier
__device__ __forceinline__ double* draws_stage_pair(const DrawLds& L, double* sm, int wv, int a, int b, int ntr, int J1, const RecipeTab& rt,
                                                    const double* __restrict__ f, const double* __restrict__ W, const double* __restrict__ prior) {
    for (int e = threadIdx.x; e < J1 * J1; e += blockDim.x) sm[DrawLds::W2(J1) + e] = W[(size_t)b * J1 * J1 + e];
    recipe_fpow(f, b, ntr, threadIdx.x, sm + L.fp2());
    return draws_stage<DRAW_CHAIN>(L, sm, wv, a, ntr, J1, rt, f, W, nullptr, nullptr, 0, prior);
}

template <bool TWO>
__global__ __launch_bounds__(256) void draws_drag_params_kernel(int ntr, int nG, int J1, int jeffreys, int Tc, int t0, int thin, int kc, int kstride,
                                                                RecipeTab rt, const long long* __restrict__ offsets, const int* __restrict__ wstart,
                                                                const int* __restrict__ wend, double* __restrict__ theta, long long* __restrict__ nacc,
                                                                double* __restrict__ sums, const double* __restrict__ f, const double* __restrict__ W,
                                                                const double* __restrict__ mu, const double* __restrict__ sinv,
                                                                const double* __restrict__ prior, const double* __restrict__ frac,
                                                                const double* __restrict__ step, const double* __restrict__ lnu,
                                                                double* __restrict__ chain, double* __restrict__ rec, double* __restrict__ fin) {
    extern __shared__ double sm[];
    const int g = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng1 = nG + 1, P = rt.P;
    const long long d0 = offsets[g], d1 = offsets[g + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;  // (workgroup-uniform: no chain for this share)
    const DrawLds L = DrawLds::drag(J1, nG, rt.nnz, P, jeffreys);
    double* wave = draws_stage_pair(L, sm, wv, wstart[g], wend[g], ntr, J1, rt, f, W, prior);
    double *Wa = sm, *Wb = sm + DrawLds::W2(J1), *fa = sm + L.fp, *fb = sm + L.fp2(), *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G;
    double *tc = wave + L.tc, *tp = wave + L.tp, *rs = wave + L.rs;
    const int* col = reinterpret_cast<int*>(sm + L.col);
    const double* pr = sm + L.pr;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    constexpr int PAIR = 2 * MARG_OUT;  // a pair of records: the start walker's, then the end walker's
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        long long na = nacc[d];
        double* oc = chain + (size_t)d * kstride * P;
        double* orec = rec + (size_t)d * kstride * PAIR;
        if (lane < P) tc[lane] = tp[lane] = theta[(size_t)d * P + lane];
        wave_lds_sync();
        int cur = 0;
        double la0 = nan, lb0 = nan, pri0 = 0.0;
        if (na >= 0) {  // (wave-uniform)
            draws_recipe_forward<TWO, 1>(rt, tp, 0, lane, ng1, J1, Wa, fa, col, th, val, Hs, Gs);
            draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, rs);
            wave_lds_sync();
            draws_recipe_forward<TWO, 1>(rt, tp, 0, lane, ng1, J1, Wb, fb, col, th, val, Hs, Gs);
            draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, rs + MARG_OUT);
            wave_lds_sync();
            la0 = rs[0];
            lb0 = rs[MARG_OUT];
            pri0 = chain_prior(P, tp, pr);
        }
        if (!__builtin_amdgcn_readfirstlane((int)(__builtin_isfinite(la0) && __builtin_isfinite(lb0)))) {  // a failed chain
            for (int k = 0; k < kc; ++k) {
                if (lane < P) oc[(size_t)k * P + lane] = nan;
                if (lane < PAIR) orec[(size_t)k * PAIR + lane] = nan;
            }
            if (lane < P) theta[(size_t)d * P + lane] = nan;
            if (lane < PAIR) fin[(size_t)d * PAIR + lane] = nan;
            if (lane < 2) sums[(size_t)d * 2 + lane] = nan;
            if (lane == 0) nacc[d] = -1;
            wave_lds_sync();
            continue;
        }
        double sa = la0 + pri0, sb = lb0 + pri0;  // the first term of the sums
        if (t0 > 0) {
            sa = sums[(size_t)d * 2];
            sb = sums[(size_t)d * 2 + 1];
        }
        int left = thin ? thin - t0 % thin : Tc + 1, k = 0;  // (thin = 0: left never reaches 0)
        for (int i = 0; i < Tc; ++i) {
            if (lane < P) tp[lane] = tc[lane] + step[((size_t)d * Tc + i) * P + lane];
            wave_lds_sync();
            bool in = true;
            for (int p = 0; p < P; ++p) {
                const double v = tp[p];
                in = in && v >= pr[p] && v <= pr[RECIPE_MAXP + p];
            }
            int acc = 0;
            double la1 = nan, lb1 = nan, pri1 = 0.0;
            if (__builtin_amdgcn_readfirstlane((int)in)) {  // (wave-uniform: the forward pass and the solve are wave-synchronous)
                double* ot = rs + (cur ^ 1) * PAIR;
                draws_recipe_forward<TWO, 1>(rt, tp, 0, lane, ng1, J1, Wa, fa, col, th, val, Hs, Gs);
                draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, ot);
                wave_lds_sync();
                la1 = ot[0];
                if (__builtin_amdgcn_readfirstlane((int)__builtin_isfinite(la1))) {  // (wave-uniform; not finite: rejected whatever the end gives)
                    draws_recipe_forward<TWO, 1>(rt, tp, 0, lane, ng1, J1, Wb, fb, col, th, val, Hs, Gs);
                    draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, ot + MARG_OUT);
                    wave_lds_sync();
                    lb1 = ot[MARG_OUT];
                }
                pri1 = chain_prior(P, tp, pr);
                acc = __builtin_amdgcn_readfirstlane((int)drag_accept(lnu[(size_t)d * Tc + i], frac[t0 + i], la1, lb1, pri1, la0, lb0, pri0));
            }
            if (acc) {
                cur ^= 1;
                la0 = la1;
                lb0 = lb1;
                pri0 = pri1;
                ++na;
                if (lane < P) tc[lane] = tp[lane];
            }
            sa = drag_sum(sa, la0, pri0);
            sb = drag_sum(sb, lb0, pri0);
            if (--left == 0) {
                left = thin;
                if (k < kc) {  // (always: the host counts the slots of the launch the same way)
                    if (lane < P) oc[(size_t)k * P + lane] = tc[lane];
                    if (lane < PAIR) orec[(size_t)k * PAIR + lane] = rs[cur * PAIR + lane];
                }
                ++k;
            }
            wave_lds_sync();  // (the next step overwrites the trial theta, th, val, H, G and the other pair of records)
        }
        if (lane < P) theta[(size_t)d * P + lane] = tc[lane];
        if (lane < PAIR) fin[(size_t)d * PAIR + lane] = rs[cur * PAIR + lane];
        if (lane < 2) sums[(size_t)d * 2 + lane] = lane ? sb : sa;
        if (lane == 0) nacc[d] = na;
        wave_lds_sync();
    }
}

// ------------------------------------------------------------------------------------------------
// Hamiltonian Monte Carlo over theta at fixed templates (eftb_draws_hmc_params): the chain kernel with leapfrog trajectories in the place of
// its random-walk steps.  Target ln pi(theta) = ln P_marg(theta) + pri(theta) as there; the gradient g = grad ln P_marg + grad pri, the first
// the bits of eftb_draws_logp_grad_params (draws_recipe_forward, draws_solve<true>, draws_grad_adjoint), the second
// -((theta_p - loc_p) sinv_p) sinv_p.  Nothing random and nothing tuned happens here: the caller supplies the momenta mom [N][Tc][P]
// (standard normals), lnu [N][Tc], the step size eps [N][Tc] of every trajectory, nleap and the lower-triangular F [N][P][P] with
// M^-1 = F F^T (the momenta live in the whitened space: kinetic energy r.r / 2).
// The chain kernel's outer shape and staging (with erow), then per chain
//   start          record and gradient of the starting theta into slot 0, its pri; ln P not finite there, or an accept count of -1 from an
//                  earlier launch: the chain has failed, NaN in its slots, theta and ratios, accept count -1
//   trajectory i   r = mom[i], k = r.r / 2, h = eps / 2; r = r + h F^T g; then nleap times: theta' = theta' + eps F r, the box test, record
//                  and gradient at theta' into the slot that is not the current one, r = r + (eps, the last time h) F^T g.  A position
//                  outside the box, or ln P or a gradient component not finite, aborts the trajectory: it is rejected and the rest of its
//                  trip runs without evaluations (wave-uniform flags from lane 0).  Otherwise
//                      ratio = ((ln P' + pri') - k') - ((ln P + pri) - k),  accept iff lnu[i] < ratio
//                  and the slot index flips on acceptance.  ratio (NaN where aborted) goes to ratio [N][Tc]
//   store, end     as the chain kernel's, per trajectory
// Lane p < P owns component p of theta', r and g.  F^T g, F r, the updates, k, grad pri and the ratio are evaluated with every operation
// rounded on its own (no contraction), sums in ascending index order, so that NumPy reproduces them bit for bit.  Every loop's trip count is
// fixed at launch.  LDS: DrawLds, DRAW_HMC.
// ------------------------------------------------------------------------------------------------
// r_p = r_p + c (F^T g)_p, (F^T g)_p = sum_{q >= p} F[q][p] g_q
__device__ __forceinline__ void hmc_kick(int P, int lane, const double* F, const double* g, double* mo, double c) {
#pragma clang fp contract(off)
    if (lane < P) {
        double acc = 0.0;
        for (int q = 0; q < P; ++q)
            if (q >= lane) acc = acc + F[q * P + lane] * g[q];
        mo[lane] = mo[lane] + c * acc;
    }
}

// theta_p = theta_p + eps (F r)_p, (F r)_p = sum_{q <= p} F[p][q] r_q
__device__ __forceinline__ void hmc_drift(int P, int lane, const double* F, const double* mo, double* t, double eps) {
#pragma clang fp contract(off)
    if (lane < P) {
        double acc = 0.0;
        for (int q = 0; q < P; ++q)
            if (q <= lane) acc = acc + F[lane * P + q] * mo[q];
        t[lane] = t[lane] + eps * acc;
    }
}

__device__ __forceinline__ double hmc_kinetic(int P, const double* mo) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int p = 0; p < P; ++p) acc = acc + mo[p] * mo[p];
    return 0.5 * acc;
}

// g_p of the target from d ln P / d theta_p: the prior's term is added where the parameter has a prior (sinv_p != 0)
__device__ __forceinline__ double hmc_grad(double gl, double t, double loc, double s) {
#pragma clang fp contract(off)
    if (s != 0.0) {
        const double q = (t - loc) * s;
        gl = gl + -(q * s);
    }
    return gl;
}

__device__ __forceinline__ double hmc_ratio(double lp1, double pri1, double k1, double lp0, double pri0, double k0) {
#pragma clang fp contract(off)
    return ((lp1 + pri1) - k1) - ((lp0 + pri0) - k0);
}

// record of the theta in t to o [MARG_OUT] and the target's gradient there to g [P] (one wave; both ordered for the wave's reads on return).
// The forward pass is the copy WHO = 2 (see draws_recipe_forward)
template <bool TWO>
__device__ __forceinline__ void hmc_eval(const RecipeTab& rt, const RecipeGradTab& gt, int lane, int nG, int J1, int jeffreys, const double* Ws, const double* fp,
                                         const int* col, const int* erow, const double* pr, const double* __restrict__ mu, const double* __restrict__ sinv,
                                         const double* t, double* th, double* val, double* Hs, double* Gs, double* o, double* g) {
    const int ng1 = nG + 1, P = rt.P;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    draws_recipe_forward<TWO, 2>(rt, t, 0, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
    const bool ok = draws_solve<true>(lane, nG, jeffreys, Gs, mu, sinv, o);
    wave_lds_sync();
    const double acc = draws_grad_adjoint(gt, lane, ng1, J1, rt.nnz, P, fp, col, erow, th, val, Hs, Gs);
    if (lane < P) g[lane] = hmc_grad(ok ? -0.5 * acc : nan, t[lane], pr[2 * RECIPE_MAXP + lane], pr[3 * RECIPE_MAXP + lane]);
    wave_lds_sync();
}

template <bool TWO>
__global__ __launch_bounds__(256) void draws_hmc_params_kernel(int ntr, int nG, int J1, int jeffreys, int Tc, int t0, int thin, int kc, int kstride, int nleap,
                                                               RecipeTab rt, RecipeGradTab gt, const long long* __restrict__ offsets, double* __restrict__ theta,
                                                               long long* __restrict__ nacc, const double* __restrict__ f, const double* __restrict__ W,
                                                               const double* __restrict__ mu, const double* __restrict__ sinv,
                                                               const double* __restrict__ prior, const double* __restrict__ mom,
                                                               const double* __restrict__ lnu, const double* __restrict__ eps,
                                                               const double* __restrict__ factor, double* __restrict__ chain, double* __restrict__ rec,
                                                               double* __restrict__ ratio) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int P = rt.P;
    const long long d0 = offsets[c], d1 = offsets[c + 1];
    if (d0 + (long long)blockIdx.y * nw >= d1) return;  // (workgroup-uniform: no chain for this share)
    const DrawLds L(DRAW_HMC, J1, nG, rt.nnz, 0, P, jeffreys);
    double* wave = draws_stage<DRAW_HMC>(L, sm, wv, c, ntr, J1, rt, f, W, gt.erow, nullptr, 0, prior);
    double *Ws = sm, *fp = sm + L.fp, *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G;
    double *tc = wave + L.tc, *tp = wave + L.tp, *rs = wave + L.rs, *gs = wave + L.gs, *mo = wave + L.mo, *Fs = wave + L.F;
    const int *col = reinterpret_cast<int*>(sm + L.col), *erow = reinterpret_cast<int*>(sm + L.erow);
    const double* pr = sm + L.pr;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long d = d0 + (long long)blockIdx.y * nw + wv; d < d1; d += (long long)gridDim.y * nw) {
        long long na = nacc[d];
        double* oc = chain + (size_t)d * kstride * P;
        double* orec = rec + (size_t)d * kstride * MARG_OUT;
        if (lane < P) tc[lane] = tp[lane] = theta[(size_t)d * P + lane];
        for (int e = lane; e < P * P; e += 64) Fs[e] = factor[(size_t)d * P * P + e];
        wave_lds_sync();
        int cur = 0;
        double lp0 = nan, pri0 = 0.0;
        if (na >= 0) {  // (wave-uniform)
            hmc_eval<TWO>(rt, gt, lane, nG, J1, jeffreys, Ws, fp, col, erow, pr, mu, sinv, tp, th, val, Hs, Gs, rs, gs);
            lp0 = rs[0];
            pri0 = chain_prior(P, tp, pr);
        }
        if (!__builtin_amdgcn_readfirstlane((int)__builtin_isfinite(lp0))) {  // a failed chain
            for (int k = 0; k < kc; ++k) {
                if (lane < P) oc[(size_t)k * P + lane] = nan;
                if (lane < MARG_OUT) orec[(size_t)k * MARG_OUT + lane] = nan;
            }
            for (int i = lane; i < Tc; i += 64) ratio[(size_t)d * Tc + i] = nan;
            if (lane < P) theta[(size_t)d * P + lane] = nan;
            if (lane == 0) nacc[d] = -1;
            wave_lds_sync();
            continue;
        }
        int left = thin - t0 % thin, k = 0;
        for (int i = 0; i < Tc; ++i) {
            const double e = eps[(size_t)d * Tc + i], h = 0.5 * e;
            if (lane < P) {
                mo[lane] = mom[((size_t)d * Tc + i) * P + lane];
                tp[lane] = tc[lane];
            }
            wave_lds_sync();
            const double k0 = hmc_kinetic(P, mo);
            wave_lds_sync();  // (every lane has read the momentum it was dealt)
            hmc_kick(P, lane, Fs, gs + cur * RECIPE_MAXP, mo, h);
            wave_lds_sync();
            double* ot = rs + (cur ^ 1) * MARG_OUT;
            double* gn = gs + (cur ^ 1) * RECIPE_MAXP;
            int bad = 0;  // (wave-uniform: the trajectory is aborted)
            for (int s = 0; s < nleap; ++s) {
                if (bad) continue;
                hmc_drift(P, lane, Fs, mo, tp, e);
                wave_lds_sync();
                bool in = true;
                for (int p = 0; p < P; ++p) {
                    const double v = tp[p];
                    in = in && v >= pr[p] && v <= pr[RECIPE_MAXP + p];
                }
                if (!__builtin_amdgcn_readfirstlane((int)in)) {
                    bad = 1;
                    continue;
                }
                // (wave-uniform from here: the forward pass, the solve and the adjoint are wave-synchronous)
                hmc_eval<TWO>(rt, gt, lane, nG, J1, jeffreys, Ws, fp, col, erow, pr, mu, sinv, tp, th, val, Hs, Gs, ot, gn);
                bool fin = __builtin_isfinite(ot[0]);
                for (int p = 0; p < P; ++p) fin = fin && __builtin_isfinite(gn[p]);
                if (!__builtin_amdgcn_readfirstlane((int)fin)) {
                    bad = 1;
                    continue;
                }
                hmc_kick(P, lane, Fs, gn, mo, s == nleap - 1 ? h : e);
                wave_lds_sync();
            }
            int acc = 0;
            double lp1 = nan, pri1 = 0.0, lr = nan;
            if (!bad) {
                lp1 = ot[0];
                pri1 = chain_prior(P, tp, pr);
                lr = hmc_ratio(lp1, pri1, hmc_kinetic(P, mo), lp0, pri0, k0);
                acc = __builtin_amdgcn_readfirstlane((int)(lnu[(size_t)d * Tc + i] < lr));
            }
            if (lane == 0) ratio[(size_t)d * Tc + i] = lr;
            if (acc) {
                cur ^= 1;
                lp0 = lp1;
                pri0 = pri1;
                ++na;
                if (lane < P) tc[lane] = tp[lane];
            }
            if (--left == 0) {
                left = thin;
                if (k < kc) {  // (always: the host counts the slots of the launch the same way)
                    if (lane < P) oc[(size_t)k * P + lane] = tc[lane];
                    if (lane < MARG_OUT) orec[(size_t)k * MARG_OUT + lane] = rs[cur * MARG_OUT + lane];
                }
                ++k;
            }
            wave_lds_sync();  // (the next trajectory overwrites the momentum, the trial theta, th, val, H, G and the other record and gradient)
        }
        if (lane < P) theta[(size_t)d * P + lane] = tc[lane];
        if (lane == 0) nacc[d] = na;
        wave_lds_sync();
    }
}

// ------------------------------------------------------------------------------------------------
// Parallel tempering over theta at fixed templates (eftb_draws_temper_params): ladders of R chains ("rungs") at inverse temperatures
// 1 >= beta_0 > ... > beta_{R-1} >= 0 that exchange states.  Chain n is rung n % R of ladder n / R; rung r targets
//     ln pi_r(theta) = beta_r ln P_marg(theta) + pri(theta)
// with ln P_marg tempered as a whole (the Gaussian priors of the marginalised parameters included) and pri, the chain kernel's prior on
// theta, not tempered.  One workgroup of R waves (blockDim = 64 R, R <= TEMPER_MAXR) works one ladder at a time, wave r its rung r, and
// loops over the ladders of its (walker, share): every wave of the workgroup has the same trip count.  Per rung the kernel is the chain
// kernel's: draws_stage, draws_recipe_forward + draws_solve<false> (the bits of eftb_draws_logp_params), chain_prior, temper_accept in the
// place of chain_accept (beta = 1: the product is exact and the bits are chain_accept's).
//   start          the record of every rung's starting theta and its pri.  The rungs publish "ln P is finite and no earlier launch has
//                  failed" through LDS and the whole workgroup decides before the step loop: one rung without, and the ladder has failed,
//                  NaN in every slot, theta and sum of every rung, accept and swap counts -1
//   step i         the chain kernel's step with beta_r ln P in the place of ln P
//   swap event     after the steps whose global number g has (g + 1) % S == 0 (S = 0: never; s0 steps remain to the launch's first event,
//                  whose global number j has the parity jpar): the pairs (r, r + 1), r = j mod 2, r + 1 < R.  Every rung publishes ln P,
//                  pri and the index of its current record slot; barrier; the wave of the lower rung of a pair decides,
//                      x = (beta_r - beta_{r+1}) (ln P_{r+1} - ln P_r),    accept iff lnus[ladder][event][r] < x          (temper_swap)
//                  from lane 0, counts it and publishes the decision; barrier; both waves of an accepted pair read the other's theta,
//                  current record, ln P and pri into registers; barrier; they write them over their own.  Temperature, accept count, swap
//                  count and sum stay with the rung (the wave)
//   after both     sum = sum + ln P of the rung's current state (untempered); the chain kernel's store after every thin-th step
//   end            theta, nacc, sums [N] and nswap [ladders][max(R - 1, 1)] (pair r: wave r) hold the state after the launch
// Barriers: two around the failed-ladder decision (the second keeps the next ladder's flags off waves that still read these) and the three
// of a swap event are the only ones behind draws_stage, and every wave of the workgroup reaches each the same number of times --
// the swap condition, the failed-ladder decision, the ladder loop and the early return for an empty share are workgroup-uniform, and a rung
// whose proposal left the box skips its evaluation, which holds no barrier.  No wave spins on another; no atomics; every value goes to
// memory by an ordinary vector store.  Every loop's trip count is fixed at launch.
// LDS: DrawLds, DRAW_CHAIN, at R waves, then the exchange xch [TEMPER_XCH]: ln P | pri | record slot | decision | alive, TEMPER_MAXR each.
// ------------------------------------------------------------------------------------------------
constexpr int TEMPER_MAXR = 8, TEMPER_XCH = 5 * TEMPER_MAXR;

__device__ __forceinline__ bool temper_accept(double lnu, double beta, double lp1, double pri1, double lp0, double pri0) {
#pragma clang fp contract(off)
    return __builtin_isfinite(lp1) && lnu < (beta * lp1 + pri1) - (beta * lp0 + pri0);
}

__device__ __forceinline__ bool temper_swap(double lnu, double beta_lo, double beta_hi, double lp_lo, double lp_hi) {
#pragma clang fp contract(off)
    return lnu < (beta_lo - beta_hi) * (lp_hi - lp_lo);
}

template <bool TWO>
__global__ __launch_bounds__(64 * TEMPER_MAXR) void draws_temper_params_kernel(
    int ntr, int nG, int J1, int jeffreys, int R, int Tc, int t0, int thin, int kc, int kstride, int S, int s0, int jpar, int nswc, RecipeTab rt,
    const long long* __restrict__ offsets, double* __restrict__ theta, long long* __restrict__ nacc, long long* __restrict__ nswap,
    double* __restrict__ sums, const double* __restrict__ f, const double* __restrict__ W, const double* __restrict__ mu,
    const double* __restrict__ sinv, const double* __restrict__ prior, const double* __restrict__ beta, const double* __restrict__ step,
    const double* __restrict__ lnu, const double* __restrict__ lnus, double* __restrict__ chain, double* __restrict__ rec) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (the rung; blockDim = 64 R)
    const int ng1 = nG + 1, P = rt.P, npair = R > 1 ? R - 1 : 1;
    const long long d0 = offsets[c], nlad = (offsets[c + 1] - d0) / R;
    if ((long long)blockIdx.y >= nlad) return;  // (workgroup-uniform: no ladder for this share)
    const DrawLds L(DRAW_CHAIN, J1, nG, rt.nnz, 0, P, jeffreys);
    double* wave = draws_stage<DRAW_CHAIN>(L, sm, wv, c, ntr, J1, rt, f, W, nullptr, nullptr, 0, prior);
    double *Ws = sm, *fp = sm + L.fp, *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G;
    double *tc = wave + L.tc, *tp = wave + L.tp, *rs = wave + L.rs;
    double* xch = sm + L.wg + R * L.wave;
    double *xl = xch, *xp = xch + TEMPER_MAXR, *xc = xch + 2 * TEMPER_MAXR, *xd = xch + 3 * TEMPER_MAXR, *xf = xch + 4 * TEMPER_MAXR;
    const int* col = reinterpret_cast<int*>(sm + L.col);
    const double* pr = sm + L.pr;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double bt = beta[wv];
    for (long long l = blockIdx.y; l < nlad; l += gridDim.y) {  // (workgroup-uniform)
        const long long d = d0 + l * R + wv, lad = (d0 + l * R) / R;
        long long na = nacc[d], ns = wv < npair ? nswap[lad * npair + wv] : 0;
        double sl = sums[d];
        double* oc = chain + (size_t)d * kstride * P;
        double* orec = rec + (size_t)d * kstride * MARG_OUT;
        if (lane < P) tc[lane] = tp[lane] = theta[(size_t)d * P + lane];
        wave_lds_sync();
        int cur = 0;
        double lp0 = nan, pri0 = 0.0;
        if (na >= 0) {  // (wave-uniform)
            draws_recipe_forward<TWO>(rt, tp, 0, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
            draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, rs);
            wave_lds_sync();
            lp0 = rs[0];
            pri0 = chain_prior(P, tp, pr);
        }
        if (lane == 0) xf[wv] = __builtin_isfinite(lp0) ? 1.0 : 0.0;
        __syncthreads();
        bool alive = true;
        for (int r = 0; r < R; ++r) alive = alive && xf[r] != 0.0;
        __syncthreads();  // (the next ladder's flags wait for every wave to have read these)
        if (!__builtin_amdgcn_readfirstlane((int)alive)) {  // a failed ladder (workgroup-uniform)
            for (int k = 0; k < kc; ++k) {
                if (lane < P) oc[(size_t)k * P + lane] = nan;
                if (lane < MARG_OUT) orec[(size_t)k * MARG_OUT + lane] = nan;
            }
            if (lane < P) theta[(size_t)d * P + lane] = nan;
            if (lane == 0) {
                nacc[d] = -1;
                sums[d] = nan;
                if (wv < npair) nswap[lad * npair + wv] = -1;
            }
            wave_lds_sync();
            continue;
        }
        int left = thin - t0 % thin, k = 0, sleft = s0, ev = 0;
        for (int i = 0; i < Tc; ++i) {
            if (lane < P) tp[lane] = tc[lane] + step[((size_t)d * Tc + i) * P + lane];
            wave_lds_sync();
            bool in = true;
            for (int p = 0; p < P; ++p) {
                const double v = tp[p];
                in = in && v >= pr[p] && v <= pr[RECIPE_MAXP + p];
            }
            int acc = 0;
            double lp1 = nan, pri1 = 0.0;
            if (__builtin_amdgcn_readfirstlane((int)in)) {  // (wave-uniform; no barrier inside)
                double* ot = rs + (cur ^ 1) * MARG_OUT;
                draws_recipe_forward<TWO>(rt, tp, 0, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
                draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, ot);
                wave_lds_sync();
                lp1 = ot[0];
                pri1 = chain_prior(P, tp, pr);
                acc = __builtin_amdgcn_readfirstlane((int)temper_accept(lnu[(size_t)d * Tc + i], bt, lp1, pri1, lp0, pri0));
            }
            if (acc) {
                cur ^= 1;
                lp0 = lp1;
                pri0 = pri1;
                ++na;
                if (lane < P) tc[lane] = tp[lane];
            }
            if (S > 0 && --sleft == 0) {  // a swap event (workgroup-uniform)
                sleft = S;
                const int par = (jpar + ev) & 1;
                const int low = ((wv - par) & 1) ? wv - 1 : wv;  // (the lower rung of this wave's pair; -1 or R - 1: none)
                const bool paired = low >= 0 && low + 1 < R;
                const int other = low == wv ? wv + 1 : low;
                if (lane == 0) {
                    xl[wv] = lp0;
                    xp[wv] = pri0;
                    xc[wv] = (double)cur;
                }
                __syncthreads();
                if (paired && low == wv) {
                    const double u = lnus[((size_t)lad * nswc + ev) * (R - 1) + low];
                    const int sw = __builtin_amdgcn_readfirstlane((int)temper_swap(u, bt, beta[wv + 1], lp0, xl[wv + 1]));
                    if (lane == 0) xd[low] = (double)sw;
                    ns += sw;
                }
                __syncthreads();
                int sw = 0;
                if (paired) sw = __builtin_amdgcn_readfirstlane((int)(xd[low] != 0.0));
                double tq = 0.0, rq = 0.0, lq = 0.0, pq = 0.0;
                if (sw) {
                    const double* ow = sm + L.wg + other * L.wave;
                    const int oslot = __builtin_amdgcn_readfirstlane((int)xc[other]);
                    if (lane < P) tq = ow[L.tc + lane];
                    if (lane < MARG_OUT) rq = ow[L.rs + oslot * MARG_OUT + lane];
                    lq = xl[other];
                    pq = xp[other];
                }
                __syncthreads();
                if (sw) {
                    if (lane < P) tc[lane] = tq;
                    if (lane < MARG_OUT) rs[cur * MARG_OUT + lane] = rq;
                    lp0 = lq;
                    pri0 = pq;
                    wave_lds_sync();
                }
                ++ev;
            }
            sl = sl + lp0;
            if (--left == 0) {
                left = thin;
                if (k < kc) {  // (always: the host counts the slots of the launch the same way)
                    if (lane < P) oc[(size_t)k * P + lane] = tc[lane];
                    if (lane < MARG_OUT) orec[(size_t)k * MARG_OUT + lane] = rs[cur * MARG_OUT + lane];
                }
                ++k;
            }
            wave_lds_sync();  // (the next step overwrites the trial theta, th, val, H, G and the other record)
        }
        if (lane < P) theta[(size_t)d * P + lane] = tc[lane];
        if (lane == 0) {
            nacc[d] = na;
            sums[d] = sl;
            if (wv < npair) nswap[lad * npair + wv] = ns;
        }
        wave_lds_sync();
    }
}

// ------------------------------------------------------------------------------------------------
// Affine-invariant ensembles over theta at fixed templates (eftb_draws_ensemble_params): the stretch move of Goodman & Weare.  Chain n is
// member n % K of ensemble n / K; members 0 ... K/2 - 1 are half 0, the rest half 1; the target is the chain kernel's ln P_marg + pri.
// One workgroup of nw waves (nw <= K/2, ENS_MAXW at most) works one ensemble at a time and loops over the ensembles of its (walker,
// share).  The members' states live in the ensemble area of the LDS behind the waves' parts (DrawLds::ens), ENS_SLOT doubles each:
// theta [RECIPE_MAXP] | record [MARG_OUT] | ln P | pri | accept count.  Member q of a half belongs to wave q % nw, which alone writes its
// slot; a wave keeps the trial theta (tp) and the trial record (rs) in its own part.  Per evaluation the kernel is the chain kernel's:
// draws_stage, draws_recipe_forward + draws_solve<false> (the bits of eftb_draws_logp_params), chain_prior, chain_accept.
//   start          the owning waves compute record and pri of every member's starting theta, pass by pass, into its slot (ln P = NaN for
//                  an accept count of -1 from an earlier launch); barrier; every wave reads all K ln P: one not finite and the ensemble
//                  has failed, NaN in every slot and theta of every member, accept counts -1; barrier
//   sweep i        half 0 against half 1, barrier, half 1 against half 0, barrier.  In a half-sweep wave w takes the members
//                  q = w, w + nw, ... of the active half, ceil((K/2) / nw) passes.  Member k with partner j = member pick[n][i] of the
//                  other half:  theta' = theta_j + z[n][i] (theta_k - theta_j)  (ens_stretch); outside the box: rejected without an
//                  evaluation; otherwise accepted iff ln P' is finite and lnq[n][i] < (ln P' + pri') - (ln P + pri); on acceptance trial
//                  theta and record go over the member's slot
//   store          after every thin-th sweep each wave stores its members' theta and record, from slots that it alone writes
//   end            theta and nacc hold the state after the launch
// Barriers: the two around the failed-ensemble decision and one behind each half-sweep are the only ones behind draws_stage, and every
// wave of the workgroup reaches each the same number of times -- the decision, the ensemble loop and the early return for an empty share are
// workgroup-uniform, every wave has the same number of passes, and a wave without a member in the last pass, or a member whose proposal left
// the box, skips its evaluation under a wave-uniform branch that holds no barrier.  Within a half-sweep writes touch only the active
// half, each slot by the wave that owns it, and reads of other waves' slots touch only the passive half: every write is across a barrier
// from every read of the same slot by another wave.  No wave spins on another; no atomics; every value goes to memory by an ordinary
// vector store.  Every loop's trip count is fixed at launch.
// LDS: DrawLds, DRAW_CHAIN, at nw waves (tc and the second record of a wave are not used), then the ensemble area [K][ENS_SLOT].
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ens_stretch(double z, double tk, double tj) {
#pragma clang fp contract(off)
    const double d = tk - tj;
    return tj + z * d;
}

template <bool TWO>
__global__ __launch_bounds__(64 * ENS_MAXW) void draws_ensemble_params_kernel(int ntr, int nG, int J1, int jeffreys, int K, int Tc, int t0, int thin, int kc,
                                                                               int kstride, RecipeTab rt, const long long* __restrict__ offsets,
                                                                               double* __restrict__ theta, long long* __restrict__ nacc,
                                                                               const double* __restrict__ f, const double* __restrict__ W,
                                                                               const double* __restrict__ mu, const double* __restrict__ sinv,
                                                                               const double* __restrict__ prior, const double* __restrict__ z,
                                                                               const int* __restrict__ pick, const double* __restrict__ lnq,
                                                                               double* __restrict__ chain, double* __restrict__ rec) {
    extern __shared__ double sm[];
    const int c = blockIdx.x, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng1 = nG + 1, P = rt.P, half = K >> 1, npass = (half + nw - 1) / nw;
    const long long d0 = offsets[c], nens = (offsets[c + 1] - d0) / K;
    if ((long long)blockIdx.y >= nens) return;  // (workgroup-uniform: no ensemble for this share)
    const DrawLds L(DRAW_CHAIN, J1, nG, rt.nnz, 0, P, jeffreys);
    double* wave = draws_stage<DRAW_CHAIN>(L, sm, wv, c, ntr, J1, rt, f, W, nullptr, nullptr, 0, prior);
    double *Ws = sm, *fp = sm + L.fp, *th = wave + L.th, *val = wave + L.val, *Hs = wave + L.H, *Gs = wave + L.G;
    double *tp = wave + L.tp, *rs = wave + L.rs;
    double* ens = sm + L.ens(nw);
    const int* col = reinterpret_cast<int*>(sm + L.col);
    const double* pr = sm + L.pr;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long l = blockIdx.y; l < nens; l += gridDim.y) {  // (workgroup-uniform)
        const long long db = d0 + l * K;
        // ---- start: the records of this wave's members
        for (int h = 0; h < 2; ++h)
            for (int ps = 0; ps < npass; ++ps) {
                const int q = wv + ps * nw;
                if (q < half) {  // (wave-uniform; no barrier inside)
                    const int k = h * half + q;
                    const long long d = db + k;
                    double* me = ens + k * ENS_SLOT;
                    const long long na = nacc[d];
                    if (lane < P) tp[lane] = me[lane] = theta[(size_t)d * P + lane];
                    wave_lds_sync();
                    double lp0 = nan, pri0 = 0.0;
                    if (na >= 0) {  // (wave-uniform)
                        draws_recipe_forward<TWO>(rt, tp, 0, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
                        draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, rs);
                        wave_lds_sync();
                        lp0 = rs[0];
                        pri0 = chain_prior(P, tp, pr);
                        if (lane < MARG_OUT) me[ENS_REC + lane] = rs[lane];
                    }
                    if (lane == 0) {
                        me[ENS_LP] = lp0;
                        me[ENS_PRI] = pri0;
                        me[ENS_NA] = (double)na;
                    }
                    wave_lds_sync();  // (the next member overwrites tp, th, val, H, G and rs)
                }
            }
        __syncthreads();
        bool alive = true;
        for (int k = 0; k < K; ++k) alive = alive && __builtin_isfinite(ens[k * ENS_SLOT + ENS_LP]);
        __syncthreads();  // (the first half-sweep, and a failed ensemble's successor, write slots that every wave must have read)
        if (!__builtin_amdgcn_readfirstlane((int)alive)) {  // a failed ensemble (workgroup-uniform)
            for (int h = 0; h < 2; ++h)
                for (int ps = 0; ps < npass; ++ps) {
                    const int q = wv + ps * nw;
                    if (q < half) {
                        const long long d = db + h * half + q;
                        double* oc = chain + (size_t)d * kstride * P;
                        double* orec = rec + (size_t)d * kstride * MARG_OUT;
                        for (int k = 0; k < kc; ++k) {
                            if (lane < P) oc[(size_t)k * P + lane] = nan;
                            if (lane < MARG_OUT) orec[(size_t)k * MARG_OUT + lane] = nan;
                        }
                        if (lane < P) theta[(size_t)d * P + lane] = nan;
                        if (lane == 0) nacc[d] = -1;
                    }
                }
            continue;
        }
        int left = thin - t0 % thin, ks = 0;
        for (int i = 0; i < Tc; ++i) {
            for (int h = 0; h < 2; ++h) {
                for (int ps = 0; ps < npass; ++ps) {
                    const int q = wv + ps * nw;
                    if (q < half) {  // (wave-uniform; no barrier inside)
                        const int k = h * half + q;
                        const size_t at = (size_t)(db + k) * Tc + i;
                        double* me = ens + k * ENS_SLOT;
                        const double* you = ens + ((1 - h) * half + pick[at]) * ENS_SLOT;
                        if (lane < P) tp[lane] = ens_stretch(z[at], me[lane], you[lane]);
                        wave_lds_sync();
                        bool in = true;
                        for (int p = 0; p < P; ++p) {
                            const double v = tp[p];
                            in = in && v >= pr[p] && v <= pr[RECIPE_MAXP + p];
                        }
                        if (__builtin_amdgcn_readfirstlane((int)in)) {  // (wave-uniform: the forward pass and the solve are wave-synchronous)
                            draws_recipe_forward<TWO>(rt, tp, 0, lane, ng1, J1, Ws, fp, col, th, val, Hs, Gs);
                            draws_solve<false>(lane, nG, jeffreys, Gs, mu, sinv, rs);
                            wave_lds_sync();
                            const double lp1 = rs[0], pri1 = chain_prior(P, tp, pr);
                            if (__builtin_amdgcn_readfirstlane((int)chain_accept(lnq[at], lp1, pri1, me[ENS_LP], me[ENS_PRI]))) {
                                const double na = me[ENS_NA] + 1.0;
                                wave_lds_sync();  // (every lane has read ln P, pri and the count of the slot)
                                if (lane < P) me[lane] = tp[lane];
                                if (lane < MARG_OUT) me[ENS_REC + lane] = rs[lane];
                                if (lane == 0) {
                                    me[ENS_LP] = lp1;
                                    me[ENS_PRI] = pri1;
                                    me[ENS_NA] = na;
                                }
                            }
                        }
                        wave_lds_sync();  // (the next member overwrites the trial theta, th, val, H, G and the trial record)
                    }
                }
                __syncthreads();  // (the half that moved is the other half's partner next)
            }
            if (--left == 0) {
                left = thin;
                if (ks < kc)  // (always: the host counts the slots of the launch the same way)
                    for (int h = 0; h < 2; ++h)
                        for (int ps = 0; ps < npass; ++ps) {
                            const int q = wv + ps * nw;
                            if (q < half) {
                                const int k = h * half + q;
                                const long long d = db + k;
                                const double* me = ens + k * ENS_SLOT;
                                if (lane < P) chain[((size_t)d * kstride + ks) * P + lane] = me[lane];
                                if (lane < MARG_OUT) rec[((size_t)d * kstride + ks) * MARG_OUT + lane] = me[ENS_REC + lane];
                            }
                        }
                ++ks;
            }
        }
        for (int h = 0; h < 2; ++h)
            for (int ps = 0; ps < npass; ++ps) {
                const int q = wv + ps * nw;
                if (q < half) {
                    const int k = h * half + q;
                    const long long d = db + k;
                    const double* me = ens + k * ENS_SLOT;
                    if (lane < P) theta[(size_t)d * P + lane] = me[lane];
                    if (lane == 0) nacc[d] = (long long)me[ENS_NA];
                }
            }
        // (no barrier: the next ensemble's starts go to slots that their own waves alone have touched since the last half-sweep's barrier)
    }
}

}  // namespace eftb
