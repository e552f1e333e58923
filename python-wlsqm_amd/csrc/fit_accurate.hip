// fit_accurate.hip — the ACCURATE numerics mode (WLSQM_HIP_STRICT=2 / wlsqm_hip_set_strict(2)) for gfx950: the mode that is meant
// to satisfy BOTH halves of the north-star target at once — derivative DOFs within 1e-10 of the reference's on every column AND a
// fit rate at the HBM roofline's scale.
//
// What it is.  The strict mode (fit_strict.hip) replays the reference's floating-point operations one for one and is 5x slower
// than the fast kernels; the fast kernels are 2.4e-10 from the reference on configs[1].  profiles/r03_attribution.txt says which of
// the fast kernels' choices cost that distance: the split neighbour sums, the reciprocal in the weights, the unscaled LDL^T — and
// that ONE choice is free: assembling only the upper triangle of the normal matrix and mirroring it (3.33e-11 against the strict
// mode's 3.36e-11 on configs[1], 1.71e-11 against 1.69e-11 on configs[4]; the V_SYM switch of the tests' CPU checker).  This kernel is therefore the
// reference's arithmetic with exactly that one change:
//
//   make_c_{2,3}D        impl.pyx:286-432, 70-269     the reference's grouping of every scaled monomial
//   Case_make_weights    infra.pyx:668-702            CORRECTLY ROUNDED quotient and root (bit-identical to IEEE / and sqrt)
//   make_A               impl.pyx:566-602             entry (j, m), m >= j: sum_k (w c_m) c_j, k ascending in ONE lane, no FMA;
//                                                     entry (m, j) := entry (j, m)   <- the one change
//   rescale_ruiz2001_c   lapackdrivers.pyx:553-623    the same sweeps with the same stop test; on a symmetric matrix the row and the
//                                                     column pass see the same numbers (DR == DC bit for bit), so one of them is run
//   dgetrf / dgetrs      lapackdrivers.pyx:1628-1665  unblocked partial-pivot LU, first maximum wins
//   solve                impl.pyx:731-846             right-hand side sums, un-scaling
//
// and its output is BIT-IDENTICAL to the CPU statement of exactly these operations that the tests hold it to (tests/test_gpu_accurate.py),
// layout- and tile-mate-independent.
//
// Where the time of the strict register kernel went, and what is different here (same bits, fewer instructions):
//   * IEEE divide = v_div_scale x2 + v_rcp + 4 fma + mul + fma + v_div_fmas + v_div_fixup (11 instructions; read from the ISA).
//     For operands whose exponents are far from the ends of the range the two scale instructions return their inputs, div_fmas is a
//     plain fma and div_fixup the identity: the remaining 8 instructions ARE the quotient (fdiv below; same operations, same
//     bits).  The weights divide every squared distance by the same max_d2: the refined reciprocal is computed once per case and a
//     quotient costs 3 instructions.  IEEE sqrt likewise: 17 -> 10 (no scaling, no class test).  Whether a case's operands are in
//     the safe range is CHECKED (squared distances, matrix entries, the running scale factors); a wave with any case outside it
//     runs the same code with the compiler's IEEE sequences instead (same bits where both apply) — never a silent approximation.
//     tools/ubench/exact_div_sqrt.hip holds the two sequences against `/` and sqrt() on 2^31 random operand pairs.
//   * the matrix is 21 / 55 sums instead of 36 / 100, the equilibration 21 / 55 quotients per sweep instead of 36 / 100 and one
//     set of roots and scale updates instead of two.
//   * the row exchanges of the LU (selects over the candidate rows: registers cannot be indexed by a lane's pivot row) are skipped
//     by a wave whose 64 cases all keep the diagonal pivot in that column — 99.9 % of configs[1]'s columns, 99.5 % of configs[4]'s.
//   * the neighbour rows of the 64 cases of a wave reach their lanes through LDS in chunks of 8 neighbours: global loads are
//     coalesced 16-byte pieces of whole 128- / 192-byte runs (the strict register kernel's lanes each read their own row: 64 cache
//     lines per load instruction), the next chunk is in flight in registers while the current one is consumed.
// One lane per case; a wave owns 64 consecutive cases.  EVERY knowns mask is taken (round 5: masks inside the polynomial's DOFs, the
// reference's default knowns = b?_F of simple.pyx:60-61 included; round 6: masks with stray bits beyond them too):
//   * the MASKED FULL system.  Known rows and columns of the assembled matrix become rows of the identity; the
//     equilibration leaves them at scale 1 (their only quotient is 1 / (1 x 1)) and never sees them in another row's maximum (their
//     quotients there are 0), the pivot search never picks them for another column (their entries are 0 and the first maximum wins)
//     and their multipliers are 0: every operation on the unknowns' entries is the reduced system's (infra.pyx:145-200 remap),
//     bit for bit, with every index a compile-time constant.
//   * the known values move to the right-hand side as the reference does it (impl.pyx:792-823): term by term into b[j], every term
//     carrying the row scale — so after the equilibration, in one more pass over the neighbours PER known DOF (the sums of two knowns
//     must not interleave: b[j] walks all neighbours of the first before the second).  The rows come back from L2 / the Infinity Cache.
//   * stray mask bits (infra.pyx:119-121: nr = no - popcount(knowns) counts them, remap does not): the reference solves for the FIRST nr
//     unknown DOFs only and never touches the others — here the others are rows of the identity like a known DOF, without an
//     elimination pass and never written (wlsqm_kernels.hpp: effective_mask; the same bits as the reduced system, as above).
// ONE LAUNCH PER CALL (round 6).  Rounds 4-5 sent a group the speculative pass could not vouch for (unsorted
// neighbours, an operand outside the safe range, the partial last group) to a REDO LIST walked by a second kernel, and cases with stray
// mask bits to a LEFTOVER LIST walked by the strict kernels: three launches per call, two of them idle in the common case, and a
// persistent per-stream counter buffer to feed them (~25 us of a 0.28 ms call on the driver's box; ADVICE r5: not safe for two host
// threads on one stream).  Now the wave that cannot vouch for its group runs the two-pass form ON THE SPOT (a wave-uniform branch inside
// the same kernel: the same code as before, the same bits), and no case is left over: no lists, no counters, no second kernel.
// 2D order 4, sensitivities, refinement and 1D fits are NOT taken here: in accurate mode they run the strict kernels (the reference's
// operations one for one, i.e. at least as close to the reference).  (Round 5's one-lane-per-case strict form of 2D order 4 with F known —
// `LANE14`: bit-identical to the strict kernels, 1 693 spilled registers, slower than the row-per-lane kernel — is gone from the library; it is
// in the history at commit c9ef97d.)
//
// THE CONTRACTED MODE (WLSQM_HIP_STRICT=3 / wlsqm_hip_set_strict(3); last_kernel "accurate-fma") is this file once more with the template
// parameter FMA = true: the accurate mode with a <- fma(b, c, a) in the neighbour sums of the matrix ((w c_m) is rounded, then fused
// with c_j) and of the right-hand side ((w f_k) rounded, fused with c_a), in the update of the trailing matrix of the LU and in the
// two substitutions — the V_SYM | V_FMA switches of the tests' CPU checker, bit for bit on every path below (tests/test_gpu_contracted.py).
// The monomials, the weights, the equilibration sweeps, the scaling, the term-by-term elimination of known DOFs, the quotients and
// the un-scaling stay rounded operation by operation.  FMA = false instantiates exactly the code it did before the parameter existed.
#include <atomic>
#include <type_traits>

#include "wlsqm_chunk.hpp"
#include "wlsqm_dispatch.hpp"
#include "wlsqm_kernels.hpp"
#include "wlsqm_strict.hpp"

#pragma clang fp contract(off)      // the reference is gcc -O2 on x86-64: no contraction; every fma() below is spelled out

// ---- compile-time switches (tools/ab_unit.sh rebuilds this unit with -DNAME=value; the table of all of them: DESIGN section 8)
#ifndef WLSQM_ACC_MINW6
#define WLSQM_ACC_MINW6 2           // waves per SIMD the kernel of the systems up to 6 unknowns is compiled for
#endif
#ifndef WLSQM_ACC_MINW10
#define WLSQM_ACC_MINW10 1          // ... of the 10-unknown systems
#endif
#ifndef WLSQM_ACC_W1
#define WLSQM_ACC_W1 2              // chunks in flight in pass 1 of the two-pass form, 2D (a chunk's few instructions do not cover the next one's loads; 3D: always 2)
#endif
#ifndef WLSQM_ACC_GRP
#define WLSQM_ACC_GRP 2             // neighbours per straight-line group of the accumulation, systems up to 6 unknowns (the size measured flat, profiles/r04b_ab_accurate.txt; the 10-unknown systems take the whole chunk)
#endif

namespace wlsqm {

namespace acc {

constexpr int CH = 8;                                                // neighbours per staged chunk
constexpr int GRP = WLSQM_ACC_GRP < CH ? WLSQM_ACC_GRP : CH;                                   // neighbours per straight-line group of the accumulation

template <int N> __host__ __device__ constexpr int utri(int i, int m) { return i * N - i * (i - 1) / 2 + (m - i); }   // i <= m < N

__host__ __device__ constexpr int minw(int NO) { return NO <= 6 ? WLSQM_ACC_MINW6 : WLSQM_ACC_MINW10; }

// a += b c and a -= b c.  FMA (the CONTRACTED mode, WLSQM_HIP_STRICT=3): ONE rounding, spelled as the builtin — the file is compiled with
// contraction off, so these are the only places where a product meets a sum unrounded (the V_FMA switch of the tests' CPU checker).
// (Macros around the accurate mode's own statements, not functions: with the sum written as a function's return value the FMA = false
// kernels came out of the register allocator with other spill counts — same operations, another order in the IR.  They read the
// template parameter `FMA` of the function they are used in — lu_solve_store and accurate_group, nowhere else — and are undefined
// again at the end of this file.)
#define WLSQM_ACC_MAC(a, b, c)  do { if constexpr (FMA) (a) = __builtin_fma((b), (c), (a)); else (a) += (b) * (c); } while (0)
#define WLSQM_ACC_NMAC(a, b, c) do { if constexpr (FMA) (a) = __builtin_fma(-(b), (c), (a)); else (a) -= (b) * (c); } while (0)

}  // namespace acc


namespace acc {

// range check of the fast equilibration sweeps: every nonzero entry of the matrix in the safe range and no zero row
template <int N>
__device__ __forceinline__ bool entries_in_range(const double (&U)[N * (N + 1) / 2]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double rowmax = 0.;
#pragma unroll
        for (int m = 0; m < N; ++m) {
            const double a = fabs(U[i <= m ? utri<N>(i, m) : utri<N>(m, i)]);
            ok = ok && (a == 0. || (a >= RANGE_LO && a <= RANGE_HI));
            rowmax = a > rowmax ? a : rowmax;
        }
        ok = ok && rowmax >= RANGE_LO;
    }
    return ok;
}

// rescale_ruiz2001_c (lapackdrivers.pyx:553-623) on the symmetric matrix: DR == DC, DRp == DCp, rs == cs bit for bit, so one
// pass per sweep.  Returns whether every running scale factor stayed in the safe range of the fast sequences.
//
// DIAG (fast path only): a sweep needs the LARGEST quotient |A[i][m]| / (DRp[i] DRp[m]) of every row, nothing else.  The matrix is
// a Gram matrix, A[i][m]^2 = c_im^2 A[i][i] A[m][m] with c_im < 1 the cosine of two weighted monomial columns, so a quotient is
// q_im = c_im sqrt(q_ii q_mm) (1 + O(2^-50)): once the DIAGONAL quotients of a sweep are within a factor 1 / c_max^2 of each other,
// no off-diagonal quotient can exceed the diagonal one of its row or of its column, every row maximum IS its diagonal quotient and
// the other N (N - 1) / 2 quotients of the sweep need not be computed — the same doubles come out, not an approximation.  c_max^2 is
// computed once per case (raw v_rcp_f64: 2^-23, covered by the 2^-16 margin below); the test is wave-uniform (every lane of the
// wave must pass: otherwise the full sweep runs, which is always right).  On BASELINE configs[1] the sweeps from the third on pass.
template <int N, class OPS, bool DIAG = false>
__device__ __forceinline__ bool ruiz_sym(const double (&U)[N * (N + 1) / 2], double (&rs)[N]) {
    using strict::ruiz_epsilon;
    double DRp[N];
    bool in_range = true;
#pragma unroll
    for (int i = 0; i < N; ++i) { rs[i] = 1.; DRp[i] = 1.; }
    double thresh = 0.;                                                // c_max^2 (1 + 2^-16); NaN / inf (a zero diagonal entry): never passes
    if constexpr (DIAG && N > 1) {
        double ra[N], cm2 = 0.;
#pragma unroll
        for (int i = 0; i < N; ++i) ra[i] = __builtin_amdgcn_rcp(U[utri<N>(i, i)]);
#pragma unroll
        for (int m = 1; m < N; ++m)
#pragma unroll
            for (int i = 0; i < m; ++i) { const double a = U[utri<N>(i, m)]; cm2 = __builtin_fmax(cm2, (a * a) * (ra[i] * ra[m])); }
        thresh = cm2 * (1. + 0x1p-16);
        if (!(thresh >= 0.)) thresh = 2.;                              // (fmax dropped a NaN: make the test fail)
    }
    auto finish = [&](double (&DR)[N]) -> bool {                       // roots, scale updates, stop test; true: converged
        double acc = 0.;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double h;
            const double s = OPS::sqrt_h(DR[i], h);
            DRp[i] *= s; rs[i] = OPS::div_by_root(rs[i], s, h);
            in_range = in_range && DRp[i] >= SCALE_LO && DRp[i] <= SCALE_HI;      // (a NaN fails it)
            const double tmp = fabs(1. - s * s);
            if (i == 0) acc = tmp; else acc = OPS::maxnum(acc, tmp);
        }
        return acc < ruiz_epsilon;                                    // (the column test sees the same numbers)
    };
    double DR[N];
    // first sweep: both running factors are 1.0, their product is 1.0 and x / 1.0 == x exactly: no quotient to compute
#pragma unroll
    for (int i = 0; i < N; ++i) DR[i] = 0.;
#pragma unroll
    for (int m = 0; m < N; ++m)
#pragma unroll
        for (int i = 0; i <= m; ++i) {
            const double q = fabs(U[utri<N>(i, m)]);
            DR[i] = OPS::maxnum(DR[i], q);
            if (i != m) DR[m] = OPS::maxnum(DR[m], q);
        }
    if (finish(DR)) return in_range;
    for (int it = 1; it < 100; ++it) {
        // diagonal quotients (needed by both forms of the sweep)
        double qlo = 0., qhi = 0.;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            // (seed of the reciprocal of DRp[i] DRp[m]: rs[i] rs[m] — every sweep multiplies DRp[i] and divides rs[i] by the same root,
            // each rounded once, so rs[i] DRp[i] = 1 +- 2 k 2^-53 after k sweeps)
            DR[i] = OPS::maxnum(0., fabs(OPS::div_seeded(U[utri<N>(i, i)], DRp[i] * DRp[i], rs[i] * rs[i])));      // (as the reference: a NaN quotient is skipped)
            if constexpr (DIAG) { qlo = i ? __builtin_fmin(qlo, DR[i]) : DR[i]; qhi = i ? __builtin_fmax(qhi, DR[i]) : DR[i]; }
        }
        bool diag_only = false;
        if constexpr (DIAG && N > 1) diag_only = __all(thresh * qhi <= qlo);      // (a NaN quotient fails it)
        if (!diag_only) {
#pragma unroll
            for (int m = 1; m < N; ++m)
#pragma unroll
                for (int i = 0; i < m; ++i) {
                    const double q = fabs(OPS::div_seeded(U[utri<N>(i, m)], DRp[i] * DRp[m], rs[i] * rs[m]));
                    DR[i] = OPS::maxnum(DR[i], q);
                    DR[m] = OPS::maxnum(DR[m], q);
                }
        }
        if (finish(DR)) break;
    }
    return in_range;
}

// apply_scaling_c (lapackdrivers.pyx:293-299), dgetrf (unblocked dgetf2 semantics, :1628-1635), dgetrs('N') and the un-scaling of
// solve (impl.pyx:827-846) for the systems up to 10 unknowns, everything in registers.  b arrives as the reference's right-hand side
// (row-scaled sums, knowns eliminated); `known`: DOFs that are not written (rows of the identity in U: see the header).  The row
// exchange is written as selects over the candidate rows; a wave none of whose cases leaves the diagonal pivot in a column skips it.
// (The 2 N quotients here are the compiler's IEEE sequences: a pivot may be anything.)
// FMA: the update of the trailing matrix and the two substitutions are a <- fma(-l, u, a) (the contracted mode); the scaling, the
// multipliers, the quotients and the un-scaling are rounded as ever.
template <int N, bool FMA>
__device__ __forceinline__ void lu_solve_store(const double (&U)[N * (N + 1) / 2], const double (&rs)[N], double (&b)[N], const unsigned known,
                                               double* fio) {
    double A[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int m = i; m < N; ++m) { const double v = U[utri<N>(i, m)] * (rs[i] * rs[m]); A[i][m] = v; A[m][i] = v; }
    int ipiv[N];
#pragma unroll
    for (int c0 = 0; c0 < N; ++c0) {
        int pv = c0; double best = fabs(A[c0][c0]), pval = A[c0][c0];
#pragma unroll
        for (int i = c0 + 1; i < N; ++i) { const double v = fabs(A[i][c0]); if (v > best) { best = v; pv = i; pval = A[i][c0]; } }
        ipiv[c0] = pv;
        if (__any(pv != c0)) {
#pragma unroll
            for (int i = c0 + 1; i < N; ++i) {
                const bool sw = (pv == i);
#pragma unroll
                for (int m = 0; m < N; ++m) { const double u = A[c0][m], v = A[i][m]; A[c0][m] = sw ? v : u; A[i][m] = sw ? u : v; }
            }
        }
        if (pval != 0.) {
            const double r = 1. / A[c0][c0];
#pragma unroll
            for (int i = c0 + 1; i < N; ++i) A[i][c0] *= r;
        }
#pragma unroll
        for (int m = c0 + 1; m < N; ++m) {
            const double u = A[c0][m];
#pragma unroll
            for (int i = c0 + 1; i < N; ++i) WLSQM_ACC_NMAC(A[i][m], A[i][c0], u);
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (__any(ipiv[i] != i)) {
#pragma unroll
            for (int q = i + 1; q < N; ++q) { const bool sw = (ipiv[i] == q); const double u = b[i], v = b[q]; b[i] = sw ? v : u; b[q] = sw ? u : v; }
        }
    }
#pragma unroll
    for (int c0 = 0; c0 < N; ++c0)
#pragma unroll
        for (int i = c0 + 1; i < N; ++i) WLSQM_ACC_NMAC(b[i], A[i][c0], b[c0]);
#pragma unroll
    for (int c0 = N - 1; c0 >= 0; --c0) {
        b[c0] /= A[c0][c0];
#pragma unroll
        for (int i = 0; i < c0; ++i) WLSQM_ACC_NMAC(b[i], A[i][c0], b[c0]);
    }
    // un-scale (impl.pyx:838-846); `fio` == nullptr: the caller stores the wave's rows as one run (b is left holding the results)
#pragma unroll
    for (int i = 0; i < N; ++i) b[i] = b[i] * rs[i];
    if (fio) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (!((known >> i) & 1u)) fio[i] = b[i];
    }
}

}  // namespace acc
// DENSE: contiguous rows xk[ncases][K][DIM], fk[ncases][K] with 16-byte aligned bases and rows (staged through LDS); otherwise the
// rows are read per lane through strict::Rows (any strides, index-based input, order buckets) — the same arithmetic, the same bits.
//
// One 64-case group.  SPEC (dense rows only): ONE pass over the neighbours for the sums.  The weights need the largest squared distance
// of the case before the first term can be summed, which is what makes the reference (and the two-pass form of this kernel) read every
// neighbourhood twice — 1.31 GB instead of 0.85 through the fabric per 1M configs[1] cases, and a first pass whose few
// instructions per neighbour cannot cover its own load latency.  Neighbour lists that come out of a k-nearest-neighbour search
// are sorted by distance (scipy's cKDTree.query, wlsqm.hip.knn: the reference's examples and every BASELINE config), so the LAST
// neighbour is the farthest: the pass runs with that guess while it also tracks the true maximum, and the guess is VERIFIED bit for
// bit afterwards.  A group with a wrong guess (unsorted neighbours: a ball query) or an operand outside the safe range of the fast
// sequences is fitted again, from scratch, by the two-pass form: speculation, never approximation.
// Returns true (wave-uniform, SPEC only) when the caller must run the two-pass form on this group; nothing has been stored then.
// FMA: the contracted mode — the neighbour sums of the matrix and of the right-hand side, the LU update and the substitutions fused
// (WLSQM_ACC_MAC / _NMAC above), every other operation of this function exactly as in the accurate mode.
template <int DIM, int ORDER, bool DENSE, bool SPEC, bool FMA>
__device__ __forceinline__ bool accurate_group(const KParams& p, const long long t0, double* const lds) {
    using namespace strict;
    using namespace acc;
    static_assert(!SPEC || DENSE, "the speculative single pass stages dense rows");
    constexpr int N = ndofs(DIM, ORDER), NE = N * (N + 1) / 2;
    constexpr unsigned FULL = (N >= 32) ? ~0u : ((1u << N) - 1u);
    using Pieces = ChunkPieces<DIM, CH>;                             // (wlsqm_chunk.hpp: which lane moves which 16-byte piece)
    constexpr int XPC = Pieces::XPC, FPC = Pieces::FPC, XCPI = Pieces::XCPI, XNI = Pieces::XNI, FCPI = Pieces::FCPI, FNI = Pieces::FNI;
    constexpr int XPITCH = CH * DIM + 2, FPITCH = CH + 2;            // doubles per staged row (+ 16 bytes: conflict-free b128 reads)
    double* const xs = lds;
    double* const fs = lds + 64 * XPITCH;

    const long long ncases = live_cases(p);
    // the speculative form moves whole 64-case groups in whole chunks only (no predicated loads in its loop): the last, partial group
    // of a launch is the clean-up kernel's (the launcher sends neighbour counts that are not a multiple of CH to the two-pass form altogether)
    if constexpr (SPEC) { if (ncases - t0 < 64) return true; }
    const int lane = threadIdx.x;
    const long long t = t0 + lane;
    const bool in_batch = SPEC ? true : t < ncases;                   // (the speculative form takes whole groups only: straight-line loads, no exec-masked blocks at the head)
    const long long j = in_batch ? (p.case_index ? p.case_index[t] : t) : 0;
    // ---- one pass over the neighbours of the wave's cases: consume(k, live, d, f) per lane, k ascending.  DENSE: chunks of CH
    // neighbours through LDS, the next chunk in flight in registers.  MASKED = false: every active lane has nk == K (wave-uniform).
    // A load instruction moves the chunks of XCPI (FCPI) whole cases, XPC (FPC) consecutive lanes per case: the lane's global
    // offset is ONE 32-bit register for every instruction and chunk (the rest of the address is wave-uniform) and its LDS position a
    // compile-time distance from the first one.
    const int K = (int)p.max_nk;
    const int Q = (K + CH - 1) / CH;
    const int nvalid = (ncases - t0 < 64) ? (int)(ncases - t0) : 64;
    const int xsub = lane % XPC, xc0 = lane / XPC, fsub = lane % FPC, fc0 = lane / FPC;
    const unsigned xrowb = (unsigned)K * DIM * 8, frowb = (unsigned)K * 8;
    const unsigned xg0 = (unsigned)xc0 * xrowb + (unsigned)xsub * 16u, fg0 = (unsigned)fc0 * frowb + (unsigned)fsub * 16u;
    const bool xlane = (XCPI * XPC >= 64) || lane < XCPI * XPC;       // (2D: every lane, and the compiler must see it — a predicated block of loads ends in a wait for all of them)
    d2_ xr[DENSE ? XNI : 1], fr[DENSE ? FNI : 1];
    // pass 1 of the two-pass form (largest squared distance) does a few instructions per neighbour: a chunk does not cover the latency of
    // the next one's loads.  It keeps W1 chunks in flight instead (their registers are free: the matrix is not live yet).
    constexpr int W1 = DENSE ? (XNI <= 8 ? WLSQM_ACC_W1 : 2) : 1;
    d2_ xw[W1][DENSE ? XNI : 1];
    const char* const xtile = DENSE ? reinterpret_cast<const char*>(p.xk + t0 * (long long)K * DIM) : nullptr;
    const char* const ftile = DENSE ? reinterpret_cast<const char*>(p.fk + t0 * (long long)K) : nullptr;
    auto fetch_into = [&](d2_ (&xr)[DENSE ? XNI : 1], int q, bool want_f) {      // global -> registers, coalesced 16-byte pieces
        if constexpr (DENSE) {
            const char* xb = xtile + (size_t)q * (CH * DIM * 8);
            const char* fb = ftile + (size_t)q * (CH * 8);
            const bool whole = SPEC || (nvalid == 64 && (q + 1) * CH <= K);     // wave-uniform: no case and no piece beyond the data
            if (whole) {
#pragma unroll
                for (int i = 0; i < XNI; ++i)
                    if (xlane && (i * XCPI + XCPI <= 64 || xc0 + i * XCPI < 64))
                        xr[i] = *reinterpret_cast<const d2_*>(xb + (size_t)i * XCPI * xrowb + xg0);
                if (want_f) {
#pragma unroll
                    for (int i = 0; i < FNI; ++i) fr[i] = *reinterpret_cast<const d2_*>(fb + (size_t)i * FCPI * frowb + fg0);
                }
            } else {
                const int xleft = (int)xrowb - q * (CH * DIM * 8), fleft = (int)frowb - q * (CH * 8);   // bytes of a row from this chunk on
#pragma unroll
                for (int i = 0; i < XNI; ++i)
                    if (xlane && xc0 + i * XCPI < nvalid && xsub * 16 < xleft)
                        xr[i] = *reinterpret_cast<const d2_*>(xb + (size_t)i * XCPI * xrowb + xg0);
                if (want_f) {
#pragma unroll
                    for (int i = 0; i < FNI; ++i)
                        if (fc0 + i * FCPI < nvalid && fsub * 16 < fleft)
                            fr[i] = *reinterpret_cast<const d2_*>(fb + (size_t)i * FCPI * frowb + fg0);
                }
            }
        }
    };
    auto fetch = [&](int q, bool want_f) { fetch_into(xr, q, want_f); };
    auto park_from = [&](const d2_ (&xr)[DENSE ? XNI : 1], bool want_f) {        // registers -> LDS rows
        if constexpr (DENSE) {
            double* xl = xs + xc0 * XPITCH + xsub * 2;
            double* fl = fs + fc0 * FPITCH + fsub * 2;
#pragma unroll
            for (int i = 0; i < XNI; ++i)
                if (xlane && (i * XCPI + XCPI <= 64 || xc0 + i * XCPI < 64)) *reinterpret_cast<d2_*>(xl + i * XCPI * XPITCH) = xr[i];
            if (want_f) {
#pragma unroll
                for (int i = 0; i < FNI; ++i) *reinterpret_cast<d2_*>(fl + i * FCPI * FPITCH) = fr[i];
            }
        }
    };
    auto park = [&](bool want_f) { park_from(xr, want_f); };
    // ---- the head of a group.  ROUND 6: everything the wave needs first is REQUESTED before any of it is looked at — the first staged chunk
    // (its addresses depend on the launch parameters alone), the cases' scalars, the centres and (speculative form) the LAST slot of every
    // row, which holds the farthest neighbour of a case with nk == K: in source order the mask, then nk, then the last neighbour's address
    // were three memory round trips in a row before the first chunk was even asked for (SQ_WAIT_INST_ANY: a quarter of the wave cycles).
    // (p.do_sens / p.iterative never reach this kernel)
    if constexpr (SPEC) fetch(0, true);
    const long long kn_raw = in_batch ? p.knowns[j * p.sknowns] : 0;
    const int nk_raw = in_batch ? p.nk[j * p.snk] : 0;
    const int wm_raw = in_batch ? p.wm[j * p.swm] : WLSQM_WEIGHT_UNIFORM;
    double xi[DIM], xlast[DIM];
    Rows<DIM> rows{};
    if constexpr (DENSE) {
#pragma unroll
        for (int m = 0; m < DIM; ++m) xi[m] = in_batch ? p.xi[j * p.sxi_j + m] : 0.;
        if constexpr (SPEC) {
#pragma unroll
            for (int m = 0; m < DIM; ++m) xlast[m] = in_batch ? p.xk[j * (long long)K * DIM + (long long)(K - 1) * DIM + m] : 0.;
        }
    } else {
        if (p.hoods) {
            const long long pj = own_point(p, j);
#pragma unroll
            for (int m = 0; m < DIM; ++m) xi[m] = in_batch ? p.S[pj * DIM + m] : 0.;
            rows = Rows<DIM>{nullptr, 0, nullptr, 0, p.hoods + j * p.shoods_j, p.S, p.F};
        } else {
#pragma unroll
            for (int m = 0; m < DIM; ++m) xi[m] = in_batch ? p.xi[j * p.sxi_j + m] : 0.;
            rows = Rows<DIM>{p.xk + j * p.sxk_j, p.sxk_k, p.fk + j * p.sfk_j, p.sfk_k, nullptr, nullptr, nullptr};
        }
    }
    // the mask: `known` = rows of the identity, never written (known DOFs, and the unknown DOFs the reference's nr leaves out when the mask
    // has stray bits: effective_mask); `elim` = the DOFs whose value moves to the right-hand side (impl.pyx:792-823)
    unsigned known = 0u, elim = 0u;
    if (in_batch) {
        unsigned long long k64, d64;
        effective_mask<N>(kn_raw, k64, d64);
        known = (unsigned)k64; elim = (unsigned)(k64 & ~d64);
    }
    const bool active = in_batch && known != FULL;                    // every DOF known: nothing to solve (impl.pyx:740-742)
    if (!__any(active)) return false;
    const int nk = active ? min(nk_raw, K) : 0;
    const bool uniform = active ? (wm_raw == WLSQM_WEIGHT_UNIFORM) : true;
    double* const fio = p.fi + j * p.sfi_j;

    // the neighbours of chunk q, staged in LDS: straight-line code for GRP neighbours at a time (all CH at once: the scheduler hoists
    // every LDS read and the kernel spills; the group size itself measured flat, profiles/r04b_ab_accurate.txt)
    auto chunk = [&](auto masked_tag, int q, bool want_f, auto&& consume) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const double* xrow = xs + lane * XPITCH;
        const double* frow = fs + lane * FPITCH;
        // (the 10-unknown systems run one wave per SIMD with registers to spare: the whole chunk at once, 0.758 against 0.809 ms)
        constexpr int GRP = N > 6 ? CH : acc::GRP;
        if (SPEC || (q + 1) * CH <= K) {
#pragma nounroll
            for (int g = 0; g < CH / GRP; ++g) {
                const double* xg = xrow + g * (GRP * DIM);
                const double* fg = frow + g * GRP;
#pragma unroll
                for (int kk = 0; kk < GRP; ++kk) {
                    const int k = q * CH + g * GRP + kk;
                    const bool live = MASKED ? (k < nk) : true;
                    double d[DIM];
#pragma unroll
                    for (int m = 0; m < DIM; ++m) { d[m] = xg[kk * DIM + m] - xi[m]; if (MASKED) d[m] = live ? d[m] : 0.; }
                    double f = want_f ? fg[kk] : 0.;
                    if (MASKED) f = live ? f : 0.;
                    consume(k, live, d, f);
                }
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < CH; ++kk) {
                const int k = q * CH + kk;
                if (k < K) {                                          // wave-uniform
                    const bool live = MASKED ? (k < nk) : true;
                    double d[DIM];
#pragma unroll
                    for (int m = 0; m < DIM; ++m) { d[m] = xrow[kk * DIM + m] - xi[m]; if (MASKED) d[m] = live ? d[m] : 0.; }
                    double f = want_f ? frow[kk] : 0.;
                    if (MASKED) f = live ? f : 0.;
                    consume(k, live, d, f);
                }
            }
        }
    };
    // (the staged passes run back to back: pass P's first chunk is requested under pass P - 1's last)
    // give_up(): wave-uniform, asked after every chunk — the speculative pass leaves as soon as its guess is refuted
    // (ONE copy of the fetch / park code for both forms of the chunk: with a loop per form the chunk in flight lived in different registers
    // in the two loops, and the compiler — which must assume a path from one loop into the other — made the ragged form's registers wait
    // for the full form's loads: `s_waitcnt vmcnt(0)` at the head of every chunk's arithmetic)
    const bool wave_full = __all(!active || nk == K);
    auto run_pass = [&](bool want_f, bool prefetched, bool more_passes, bool next_want_f, auto&& consume, auto&& give_up) {
        if constexpr (DENSE) {
            if (!prefetched) fetch(0, want_f);
            for (int q = 0; q < Q; ++q) {
                __syncthreads();                                      // the previous chunk has been read by every lane
                park(want_f);
                __syncthreads();
                if (q + 1 < Q) fetch(q + 1, want_f);
                else if (more_passes) fetch(0, next_want_f);
                if (wave_full) chunk(std::false_type{}, q, want_f, consume); else chunk(std::true_type{}, q, want_f, consume);
                if (give_up()) break;
            }
        } else {
            for (int k = 0; k < nk; ++k) {
                double d[DIM];
                rows.offset(k, xi, d);
                consume(k, true, d, want_f ? rows.value(k) : 0.);
            }
        }
    };
    // the same with W1 chunks in flight (coordinates only: pass 1); the next pass's first chunk is requested under the last window
    auto run_pass_windowed = [&](auto masked_tag, bool next_want_f, auto&& consume) {
        if constexpr (DENSE) {
            for (int q0 = 0; q0 < Q; q0 += W1) {
#pragma unroll
                for (int w = 0; w < W1; ++w)
                    if (q0 + w < Q) fetch_into(xw[w], q0 + w, false);
                if (q0 + W1 >= Q) fetch(0, next_want_f);
#pragma unroll
                for (int w = 0; w < W1; ++w) {
                    if (q0 + w < Q) {
                        __syncthreads();
                        park_from(xw[w], false);
                        __syncthreads();
                        chunk(masked_tag, q0 + w, false, consume);
                    }
                }
            }
        } else {
            for (int k = 0; k < nk; ++k) {
                double d[DIM];
                rows.offset(k, xi, d);
                consume(k, true, d, 0.);
            }
        }
    };
    auto pass_until = [&](bool want_f, bool prefetched, bool more_passes, bool next_want_f, auto&& consume, auto&& give_up) {
        run_pass(want_f, prefetched, more_passes, next_want_f, consume, give_up);
    };
    auto pass = [&](bool want_f, bool prefetched, bool more_passes, bool next_want_f, auto&& consume) {
        pass_until(want_f, prefetched, more_passes, next_want_f, consume, [] { return false; });
    };
    auto pass_windowed = [&](bool next_want_f, auto&& consume) {
        if (wave_full) run_pass_windowed(std::false_type{}, next_want_f, consume);
        else run_pass_windowed(std::true_type{}, next_want_f, consume);
    };

    // the upper triangle U of the normal matrix and the right-hand side sums
    double U[NE], b[N];
#pragma unroll
    for (int e = 0; e < NE; ++e) U[e] = 0.;
#pragma unroll
    for (int i = 0; i < N; ++i) b[i] = 0.;
    // make_A (impl.pyx:566-602) and the right-hand side sums of solve (impl.pyx:768-787): one neighbour's terms
    auto add_terms = [&](const double (&c)[N], double w, double f) __attribute__((always_inline)) {
        const double wf = w * f;
#pragma unroll
        for (int om = 0; om < N; ++om) {
            const double wc = w * c[om];
#pragma unroll
            for (int oj = 0; oj <= om; ++oj) WLSQM_ACC_MAC(U[utri<N>(oj, om)], wc, c[oj]);
        }
#pragma unroll
        for (int oj = 0; oj < N; ++oj) WLSQM_ACC_MAC(b[oj], wf, c[oj]);
    };
    // Known DOFs of the masked full system (the header): rows of the identity, right-hand side 0 (a wave-uniform test: the common
    // wave has none).
    const bool any_known = __any(active && known != 0u);
    auto mask_knowns = [&]() __attribute__((always_inline)) {
        if (any_known) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
#pragma unroll
                for (int m = i; m < N; ++m) {
                    const bool kk = ((known >> i) | (known >> m)) & 1u;
                    U[utri<N>(i, m)] = kk ? (i == m ? 1. : 0.) : U[utri<N>(i, m)];
                }
                b[i] = ((known >> i) & 1u) ? 0. : b[i];
            }
        }
    };
    // solve, impl.pyx:792-823: b[j] = row_scale[j] * sum, then for every known DOF om (ascending) and every neighbour k (ascending)
    // b[j] -= fi[om] * w[k] * c[k, om] * c[k, j] * row_scale[j], term by term.  One pass over the neighbours per known DOF of the wave's
    // most-masked case; a lane without a known in this round subtracts (0 * w * c * c * rs) = 0 from a sum that is never -0.
    // weight_of: the pass's weight, the same rounding sequence as in the accumulation.  All barriers inside: every lane takes part.
    auto eliminate = [&](const double (&rs)[N], auto&& weight_of) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < N; ++i) b[i] = rs[i] * b[i];
        if (!any_known) return;
        unsigned rem = active ? elim : 0u;
        while (__any(rem != 0u)) {                                    // wave-uniform
            const bool has = rem != 0u;
            const int om = has ? (__ffs(rem) - 1) : 0;
            rem &= rem - 1u;
            const double fv = has ? fio[om] : 0.;
            const bool only_f = __all(!has || om == 0);               // c[k, 0] = 1: the product with it is exact and skipped
            pass(false, false, false, false, [&](int, bool live, const double (&d)[DIM], double) {
                double c[N];
                const double d2 = make_c<DIM, ORDER>(d, c);
                double w = weight_of(d2);
                w = live ? w : 0.;
                double t = fv * w;
                if (!only_f) t = t * pick<N>(c, om);
#pragma unroll
                for (int i = 0; i < N; ++i) b[i] -= t * c[i] * rs[i];
            });
        }
#pragma unroll
        for (int i = 0; i < N; ++i) b[i] = ((known >> i) & 1u) ? 0. : b[i];
    };
    auto solve_store = [&](const double (&rs)[N]) __attribute__((always_inline)) {
        // A full group of cases without a known DOF and contiguous fi rows: the wave's 64 rows are ONE run of 64 N doubles; they go
        // through LDS (the staging rows are free: the last pass is over) and leave as whole 16-byte pieces, non-temporal — separate
        // 8-byte stores at a row pitch are partial-sector writes (fit_stage.hip: -2.5 % on configs[1]).  Wave-uniform choice.
        // (systems up to 6 unknowns: the 10-unknown kernels are at their 512 registers and paid for it with spills in their sweeps)
        const bool run = DENSE && N <= 6 && (64 * N) % 2 == 0 && (N * 64 * 8 <= (int)sizeof(double) * (64 * XPITCH + 64 * FPITCH)) && nvalid == 64 &&
                         !p.case_index && p.sfi_j == N && ((reinterpret_cast<uintptr_t>(p.fi) & 15u) == 0) && __all(active && known == 0u);
        if (active) lu_solve_store<N, FMA>(U, rs, b, known, run ? nullptr : fio);
        if (run) {
            __syncthreads();                                          // the last chunk has been read
#pragma unroll
            for (int i = 0; i < N; ++i) lds[lane * N + i] = b[i];
            __syncthreads();
            d2_* out = reinterpret_cast<d2_*>(p.fi + t0 * N);
            const d2_* src = reinterpret_cast<const d2_*>(lds);
#pragma unroll
            for (int q = lane; q < 64 * N / 2; q += 64) __builtin_nontemporal_store(src[q], &out[q]);
        }
    };
    if constexpr (SPEC) {
        // ---- the speculative single pass (see above): guess = squared distance of the last neighbour, same operations as make_c
        double guess = 0.;
        if (active && nk > 0) {
            if (nk != K) {                                            // a ragged case: its last neighbour sits elsewhere in the row
                const double* q = p.xk + j * (long long)K * DIM + (long long)(nk - 1) * DIM;
#pragma unroll
                for (int m = 0; m < DIM; ++m) xlast[m] = q[m];
            }
            double dg[DIM], cg[N];
#pragma unroll
            for (int m = 0; m < DIM; ++m) dg[m] = xlast[m] - xi[m];
            guess = make_c<DIM, ORDER>(dg, cg);
        }
        double rg = 0., max_d2 = 0., min_d2 = RANGE_HI;
        auto weight_of = [&](double d2) __attribute__((always_inline)) {
            const double tmp = 1. - FastOps::sqrt(div_by(d2, guess, rg));
            return uniform ? 1. : weights_alpha + weights_beta * tmp * tmp;
        };
        // ROUND 6: a wave whose guess is refuted (unsorted neighbours — a ball query — show it within the first chunk) does not leave for
        // another kernel any more: it finds the true maxima in a pass of its own (coordinates only, a few instructions per neighbour) and
        // runs THE SAME sums again with them — one copy of the code, executed twice, as the fast kernels do it (fit_stage.hip).  A lane
        // whose guess was right gets the same bits again.  1M configs[1] cases with shuffled rows: 0.63 -> 0.3x ms.
        bool second = false;
#pragma nounroll
        for (;;) {
#pragma unroll
            for (int e = 0; e < NE; ++e) U[e] = 0.;
#pragma unroll
            for (int i = 0; i < N; ++i) b[i] = 0.;
            max_d2 = 0.; min_d2 = RANGE_HI;
            rg = rcp_refined(guess);
            pass_until(true, true, false, false, [&](int, bool live, const double (&d)[DIM], double f) {
                double c[N];
                const double d2 = make_c<DIM, ORDER>(d, c);
                if (live) { max_d2 = __builtin_fmax(max_d2, d2); min_d2 = __builtin_fmin(min_d2, d2); }
                double w = weight_of(d2);
                w = live ? w : 0.;
                add_terms(c, w, f);
            }, [&] { return !second && __any(active && !uniform && max_d2 > guess); });
            if (second || !__any(active && !uniform && max_d2 != guess)) break;      // (a NaN distance: fmax drops it, the sum test below sees it)
            // the largest squared distance of every case, the reference's way (make_c_nD: `if d2 > max_d2`).  Every lane walks ITS OWN row
            // (plain loads, a handful of registers: staged through LDS like the sums, this pass made the whole kernel — the sorted input's
            // pass too — spill: 217 registers without it, 256 + 6..91 spilled with it); the rows come from L2, the abandoned pass has just
            // asked for their first chunk and the sums will ask for all of them again
            double m2 = 0.;
            {
                const double* row = p.xk + j * (long long)K * DIM;
#pragma nounroll
                for (int k = 0; k < nk; ++k) {
                    double d[DIM], c[N];
#pragma unroll
                    for (int m = 0; m < DIM; ++m) d[m] = row[k * DIM + m] - xi[m];
                    const double d2 = make_c<DIM, ORDER>(d, c);
                    if (d2 > m2) m2 = d2;
                }
            }
            __syncthreads();                                          // (the abandoned pass's chunk has been read by every lane)
            fetch(0, true);
            guess = m2;
            second = true;
        }
        const double first = U[0];                                    // a finite sum of the pass (NaN test)
        // vouch for the case: the guess WAS the largest squared distance (bit for bit), every squared distance in the safe range
        // of the fast quotient and root (fmax / fmin drop a NaN distance: the sum test catches it), every matrix entry and every
        // running scale factor of the equilibration too
        bool sure = !active || ((uniform || (max_d2 == guess && min_d2 >= RANGE_LO && max_d2 <= RANGE_HI)) && nk > 0 &&
                                (first - first == 0.));
        mask_knowns();
        sure = sure && (!active || entries_in_range<N>(U));
        double rs[N];
#pragma unroll
        for (int i = 0; i < N; ++i) rs[i] = 1.;
        if (__all(sure)) sure = !active || ruiz_sym<N, FastOps, true>(U, rs);
        if (!__all(sure)) return true;                                // wave-uniform: the whole group again, with the IEEE sequences
        eliminate(rs, weight_of);
        solve_store(rs);
        return false;
    } else {
        // ---- pass 1 (make_c_nD, first half): the largest squared distance; the smallest too, for the range check of the fast weights
        double max_d2 = 0., min_d2 = RANGE_HI;
        pass_windowed(true, [&](int, bool live, const double (&d)[DIM], double) {
            double c[N];
            const double d2 = make_c<DIM, ORDER>(d, c);
            if (live) { if (d2 > max_d2) max_d2 = d2; if (!(d2 >= min_d2)) min_d2 = d2; }      // (a NaN distance lands in min_d2)
        });
        // fast weights: every squared distance of the case in the safe range (a neighbour AT the centre, a NaN or an empty
        // neighbourhood fail it and take the IEEE sequences); uniform weighting computes no quotient at all
        const bool w_ok = !active || uniform || (min_d2 >= RANGE_LO && max_d2 <= RANGE_HI && nk > 0);
        const bool fast_w = __all(w_ok);

        // ---- pass 2 (make_A, right-hand side sums), equilibration (fast sequences where every operand is in their safe range, the IEEE
        // sequences for the whole wave otherwise: the same bits where both apply), knowns, scaling, LU, solve
        auto rest = [&](auto ops_tag) __attribute__((always_inline)) {
            using OPS = decltype(ops_tag);
            const double rmax = OPS::rcp_of(max_d2);
            auto weight_of = [&](double d2) __attribute__((always_inline)) {
                const double tmp = 1. - OPS::sqrt(OPS::div_r(d2, max_d2, rmax));
                return uniform ? 1. : weights_alpha + weights_beta * tmp * tmp;
            };
            pass(true, true, false, false, [&](int, bool live, const double (&d)[DIM], double f) {
                double c[N];
                const double d2 = make_c<DIM, ORDER>(d, c);
                double w = weight_of(d2);
                w = live ? w : 0.;
                add_terms(c, w, f);
            });
            mask_knowns();
            double rs[N];
#pragma unroll
            for (int i = 0; i < N; ++i) rs[i] = 1.;
            bool r_ok = !active || entries_in_range<N>(U), fast_done = false;
            if (__all(r_ok)) { r_ok = !active || ruiz_sym<N, FastOps, false>(U, rs); fast_done = true; }
            if (!fast_done || !__all(r_ok)) { if (active) (void)ruiz_sym<N, IeeeOps, false>(U, rs); }
            eliminate(rs, weight_of);
            solve_store(rs);
        };
        if (fast_w) rest(FastOps{}); else rest(IeeeOps{});
        return false;
    }
}

// LDS of a one-wave workgroup, in doubles: the staging rows
template <int DIM, bool DENSE>
__host__ __device__ constexpr int acc_lds_doubles() {
    constexpr int stage = DENSE ? 64 * (acc::CH * DIM + 2) + 64 * (acc::CH + 2) : 0;
    return stage > 2 ? stage : 2;
}

// SPEC: the speculative form.  status[g] = 1: the wave could not vouch for group g (an operand outside the safe range of the fast
// sequences): the clean-up kernel behind this one fits it again with the IEEE sequences.  A workgroup takes the groups blockIdx.x,
// blockIdx.x + gridDim.x, ...
template <int DIM, int ORDER, bool DENSE, bool SPEC, bool FMA>
__global__ __launch_bounds__(64, acc::minw(ndofs(DIM, ORDER))) void fit_accurate_kernel(const KParams p, const long long ngroups, unsigned char* const status) {
    __shared__ __attribute__((aligned(16))) double lds[acc_lds_doubles<DIM, DENSE>()];
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const bool again = accurate_group<DIM, ORDER, DENSE, SPEC, FMA>(p, g * 64, lds);
        if constexpr (SPEC) { if (threadIdx.x == 0) status[g] = again ? 1 : 0; }
        if (DENSE) __syncthreads();                                   // the LDS is reused by the next group
    }
}

// the groups the speculative kernel could not vouch for (none in the common case: ~2 us of idle waves, tools/ubench/launch_gap.hip):
// a small grid looks at the status bytes, 64 groups per wave and step
template <int DIM, int ORDER, bool FMA>
__global__ __launch_bounds__(64, acc::minw(ndofs(DIM, ORDER))) void fit_accurate_cleanup_kernel(const KParams p, const long long ngroups, const unsigned char* const status) {
    __shared__ __attribute__((aligned(16))) double lds[acc_lds_doubles<DIM, true>()];
    for (long long g0 = (long long)blockIdx.x * 64; g0 < ngroups; g0 += (long long)gridDim.x * 64) {
        const long long g = g0 + threadIdx.x;
        unsigned long long todo = __ballot(g < ngroups && status[g] != 0);
        while (todo) {                                                // wave-uniform
            const int q = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            (void)accurate_group<DIM, ORDER, true, false, FMA>(p, (g0 + q) * 64, lds);
            __syncthreads();                                          // the LDS is reused by the next group
        }
    }
}

template <int DIM, int ORDER, bool FMA>
static int launch_accurate(const KParams& p, hipStream_t stream) {
    const long long groups = (p.ncases + 63) / 64;
    if (groups <= 0) return WLSQM_OK;
    if (groups > 0x3fffffffLL) { set_error("too many cases for one launch"); return WLSQM_EVALUE; }
    const long long K = p.max_nk;
    const bool dense = !p.hoods && !p.case_index && p.xk && p.fk && K >= 2 && K % 2 == 0 && dense_rows(DIM, p, K) &&
                       !env_present("WLSQM_HIP_ACCURATE_NO_STAGE");
    const bool nospec = env_first("WLSQM_HIP_ACCURATE_NO_SPEC") == '1';      // A/B and tests: the two-pass form for every group
    if (dense && K % acc::CH == 0 && !nospec) {
        // one status byte per group, written by the speculative kernel for EVERY group: no clearing, no counters, no state between calls
        // (round 5's work lists with their alternating counter sets are gone)
        CallScratch cs;
        int rc = call_scratch_acquire(&cs, (size_t)groups, stream);
        if (rc != WLSQM_OK) return rc;
        unsigned char* const status = static_cast<unsigned char*>(cs.p);
        hipLaunchKernelGGL((fit_accurate_kernel<DIM, ORDER, true, true, FMA>), dim3((unsigned)groups), dim3(64), 0, stream, p, groups, status);
        hipError_t le = hipGetLastError();
        if (le == hipSuccess) {
            const long long want = (groups + 63) / 64, resident = 512LL * acc::minw(ndofs(DIM, ORDER));
            hipLaunchKernelGGL((fit_accurate_cleanup_kernel<DIM, ORDER, FMA>), dim3((unsigned)(want < resident ? want : resident)), dim3(64), 0, stream, p, groups, status);
            le = hipGetLastError();
        }
        rc = call_scratch_release(&cs, stream);
        if (le != hipSuccess) return hip_fail(le, "fit_accurate_kernel");
        return rc;
    }
    if (dense)
        hipLaunchKernelGGL((fit_accurate_kernel<DIM, ORDER, true, false, FMA>), dim3((unsigned)groups), dim3(64), 0, stream, p, groups, (unsigned char*)nullptr);
    else
        hipLaunchKernelGGL((fit_accurate_kernel<DIM, ORDER, false, false, FMA>), dim3((unsigned)groups), dim3(64), 0, stream, p, groups, (unsigned char*)nullptr);
    WLSQM_HIP_CHECK(hipGetLastError());
    return WLSQM_OK;
}

// Accurate mode, basic fits of the 2D / 3D systems up to 10 unknowns: EVERY case of the call is fitted here — one kernel, and behind
// it a clean-up kernel that is idle unless a group's operands left the safe range of the fast sequences.
// *handled = false: the shape or the call has no accurate kernel (1D, 2D order 4, 3D orders 3-4, sensitivities, refinement) and the
// strict kernels take every case.  FMA: the contracted mode's instantiations (launch_fit_strict picks: contracted_mode()).
template <bool FMA>
int launch_fit_accurate(int dimension, int order, const KParams& p, hipStream_t stream, bool* handled) {
    *handled = false;
    if (p.do_sens || p.iterative) return WLSQM_OK;
#define CASE(D, O) if (dimension == D && order == O) { *handled = true; return launch_accurate<D, O, FMA>(p, stream); }
    CASE(2, 0) CASE(2, 1) CASE(2, 2) CASE(2, 3)
    CASE(3, 0) CASE(3, 1) CASE(3, 2)
#undef CASE
    return WLSQM_OK;
}
template int launch_fit_accurate<false>(int, int, const KParams&, hipStream_t, bool*);
template int launch_fit_accurate<true>(int, int, const KParams&, hipStream_t, bool*);

}  // namespace wlsqm

#undef WLSQM_ACC_MAC
#undef WLSQM_ACC_NMAC
