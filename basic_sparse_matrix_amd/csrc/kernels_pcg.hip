// kernels_pcg.hip -- preconditioned conjugate gradients on a kept nd factor
// (bsm_nd_factor_solve_pcg, gfx950): S x = b with S the mirrored lower
// triangle of a (sym_obtain) and M^-1 the factor's A-system solve in the
// factor's dtype; everything else in f64. Every column is its own CG:
//   x_0, r_0 = b - S x_0                      refine's first iterate, by refine's kernels
//   z = M^-1 r                                refine_scale_cast + the nd solve
//   r . z, q . z; beta, rho; p = z + beta p   pcg_dots, pcg_judge_beta, pcg_update_p
//   q = S p, p . q; alpha                     pcg_spmv_dot, pcg_judge_alpha
//   x += alpha p, r -= alpha q; omega         pcg_step_xr, pcg_judge_norms
//   omega <= tol: the true residual decides   refine_resid, pcg_judge_norms, pcg_take_r
// The solve opens the step instead of closing it (the same sequence as
// "solve, beta, p" at the end of the step before), so none is spent after the
// last step. beta needs both dots of the whole column, so the dots and p = z +
// beta p are two kernels with the one-workgroup judge between them: z is read
// twice (n k values of the factor's dtype) and no kernel waits on another.
// The dots are sums of per-workgroup partials whose number and order depend
// on n and S alone, the maxima are taken on bit patterns, there are no
// floating-point atomics: column j's bits depend neither on k nor on the other
// columns, and the same call gives the same bits. A column that has stopped is
// skipped by its flag in every kernel.
#include <algorithm>
#include <vector>

#include "bsm_internal.hpp"
#include "pcg_rule.hpp"

namespace bsm {
namespace {

inline unsigned pcg_blocks(uint64_t n, unsigned per_block) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, REFINE_MAX_BLOCKS));
}

// KC contiguous f64 of a row: one or two 16-byte accesses for KC = 2 and 4
template <int KC>
__device__ __forceinline__ void load_kc(const double* __restrict__ p, double (&v)[KC]) {
    if constexpr (KC == 1) {
        v[0] = p[0];
    } else {
#pragma unroll
        for (int c = 0; c < KC; c += 2) {
            const double2 t = *reinterpret_cast<const double2*>(p + c);
            v[c] = t.x;
            v[c + 1] = t.y;
        }
    }
}

// Q = S P and part[block][j] = the workgroup's share of p_j . q_j. The lane
// layout of refine_resid: G lanes per row take the row's entries lane, lane +
// G, ... in stored order, explicit fma, and meet in a fixed xor tree; a
// group's lane 0 adds p q of its rows in row order, and the groups' sums are
// added in group order.
template <typename TA, int G, int KC>
__global__ __launch_bounds__(256) void pcg_spmv_dot(int64_t n, int64_t k, const int64_t* __restrict__ rp,
                                                    const int32_t* __restrict__ col, const TA* __restrict__ val,
                                                    const double* __restrict__ P, double* __restrict__ Q,
                                                    const PcgCol* __restrict__ st, double* __restrict__ part) {
    constexpr int GROUPS = 256 / G;
    __shared__ double sh[GROUPS][KC];
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    for (int64_t j0 = 0; j0 < k; j0 += KC) {
        bool on[KC], any = false;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            on[c] = st[j0 + c].active != 0;
            any = any || on[c];
        }
        if (!any) continue;  // the same for every thread
        double dot[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) dot[c] = 0.0;
        for (int64_t row0 = (int64_t)blockIdx.x * GROUPS; row0 < n; row0 += (int64_t)gridDim.x * GROUPS) {
            const int64_t row = row0 + grp;
            double acc[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) acc[c] = 0.0;
            if (row < n) {
                const int64_t e1 = rp[row + 1];
                for (int64_t e = rp[row] + lane; e < e1; e += G) {
                    const double v = (double)val[e];
                    double pv[KC];
                    load_kc<KC>(P + (int64_t)col[e] * k + j0, pv);
#pragma unroll
                    for (int c = 0; c < KC; ++c) acc[c] = fma(v, pv[c], acc[c]);
                }
            }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
#pragma unroll
                for (int c = 0; c < KC; ++c) acc[c] += __shfl_xor(acc[c], o);
            }
            if (lane == 0 && row < n) {
                double pv[KC];
                load_kc<KC>(P + row * k + j0, pv);
#pragma unroll
                for (int c = 0; c < KC; ++c)
                    if (on[c]) {
                        Q[row * k + j0 + c] = acc[c];
                        dot[c] = fma(pv[c], acc[c], dot[c]);
                    }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < KC; ++c) sh[grp][c] = dot[c];
        }
        __syncthreads();
        if ((int)threadIdx.x < KC && st[j0 + threadIdx.x].active) {
            double sum = 0.0;
            for (int g = 0; g < GROUPS; ++g) sum += sh[g][threadIdx.x];
            part[(int64_t)blockIdx.x * k + j0 + threadIdx.x] = sum;
        }
        __syncthreads();
    }
}

// x += alpha p, r -= alpha q on the active columns; part[block][0][j] = max
// |r_j|, part[block][1][j] = max |x_j| over the workgroup's rows (as bits).
// A thread takes the KC contiguous columns of a row.
template <int KC>
__global__ __launch_bounds__(256) void pcg_step_xr(int64_t n, int64_t k, const double* __restrict__ P,
                                                   const double* __restrict__ Q, double* __restrict__ X,
                                                   double* __restrict__ R, const PcgCol* __restrict__ st,
                                                   ull* __restrict__ part) {
    __shared__ ull sh[4][2 * KC];
    const int wave = threadIdx.x / 64;
    for (int64_t j0 = 0; j0 < k; j0 += KC) {
        bool on[KC], any = false;
        double alpha[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            on[c] = st[j0 + c].active != 0;
            alpha[c] = st[j0 + c].alpha;
            any = any || on[c];
        }
        if (!any) continue;
        ull m[2 * KC];
#pragma unroll
        for (int c = 0; c < 2 * KC; ++c) m[c] = 0;
        for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
            const int64_t at = row * k + j0;
            double p[KC], q[KC], x[KC], r[KC];
            load_kc<KC>(P + at, p);
            load_kc<KC>(Q + at, q);
            load_kc<KC>(X + at, x);
            load_kc<KC>(R + at, r);
#pragma unroll
            for (int c = 0; c < KC; ++c)
                if (on[c]) {
                    x[c] = fma(alpha[c], p[c], x[c]);
                    r[c] = fma(-alpha[c], q[c], r[c]);
                    X[at + c] = x[c];
                    R[at + c] = r[c];
                    m[c] = umax(m[c], abs_bits(r[c]));
                    m[KC + c] = umax(m[KC + c], abs_bits(x[c]));
                }
        }
#pragma unroll
        for (int c = 0; c < 2 * KC; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m[c] = umax(m[c], (ull)__shfl_xor((long long)m[c], o));
        }
        if (threadIdx.x % 64 == 0) {
#pragma unroll
            for (int c = 0; c < 2 * KC; ++c) sh[wave][c] = m[c];
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * KC) {
            const int which = threadIdx.x / KC, c = threadIdx.x % KC;
            if (st[j0 + c].active)
                part[((int64_t)blockIdx.x * 2 + which) * k + j0 + c] =
                    umax(umax(sh[0][threadIdx.x], sh[1][threadIdx.x]), umax(sh[2][threadIdx.x], sh[3][threadIdx.x]));
        }
        __syncthreads();
    }
}

// After the solve: z = scale W. part[block][0][j] = the workgroup's share of
// r_j . z_j, part[block][1][j] of q_j . z_j: a thread adds its rows in row
// order, a wave's lanes meet in a fixed xor tree, the four waves in order.
template <typename TF, int KC>
__global__ __launch_bounds__(256) void pcg_dots(int64_t n, int64_t k, const TF* __restrict__ W,
                                                const double* __restrict__ R, const double* __restrict__ Q,
                                                const PcgCol* __restrict__ st, double* __restrict__ part) {
    __shared__ double sh[4][2 * KC];
    const int wave = threadIdx.x / 64;
    for (int64_t j0 = 0; j0 < k; j0 += KC) {
        bool on[KC], any = false;
        double scale[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            on[c] = st[j0 + c].active != 0;
            scale[c] = st[j0 + c].scale;
            any = any || on[c];
        }
        if (!any) continue;
        double d[2 * KC];
#pragma unroll
        for (int c = 0; c < 2 * KC; ++c) d[c] = 0.0;
        for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
            const int64_t at = row * k + j0;
            double r[KC], q[KC];
            load_kc<KC>(R + at, r);
            load_kc<KC>(Q + at, q);
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const double z = scale[c] * (double)W[at + c];
                d[c] = fma(r[c], z, d[c]);
                d[KC + c] = fma(q[c], z, d[KC + c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 2 * KC; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) d[c] += __shfl_xor(d[c], o);
        }
        if (threadIdx.x % 64 == 0) {
#pragma unroll
            for (int c = 0; c < 2 * KC; ++c) sh[wave][c] = d[c];
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * KC) {
            const int which = threadIdx.x / KC, c = threadIdx.x % KC;
            if (st[j0 + c].active)
                part[((int64_t)blockIdx.x * 2 + which) * k + j0 + c] =
                    ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
        }
        __syncthreads();
    }
}

// p = z + beta p on the active columns (p = z where beta is 0: the first
// direction and a restart's, whatever p holds)
template <typename TF>
__global__ __launch_bounds__(256) void pcg_update_p(int64_t n, int64_t k, const TF* __restrict__ W,
                                                    const PcgCol* __restrict__ st, double* __restrict__ P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k) return;
    const PcgCol& c = st[i % k];
    if (!c.active) return;
    const double z = c.scale * (double)W[i];
    P[i] = c.beta == 0.0 ? z : fma(c.beta, P[i], z);
}

// r_j := the true residual, on the columns whose verification failed
__global__ __launch_bounds__(256) void pcg_take_r(int64_t n, int64_t k, const double* __restrict__ Rt,
                                                  const PcgCol* __restrict__ st, double* __restrict__ R) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k) return;
    const PcgCol& c = st[i % k];
    if (c.active && c.restart) R[i] = Rt[i];
}

// x in a's dtype
template <typename TA>
__global__ __launch_bounds__(256) void pcg_finish(int64_t n, int64_t k, const double* __restrict__ X,
                                                  const PcgCol* __restrict__ st, TA* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k) return;
    x[i] = st[i % k].zero ? (TA)0 : (TA)X[i];
}

// ---- the one-workgroup judges ------------------------------------------------
// the sum of part[b * stride + idx], b < nb, in index order (thread 0's return)
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int nb, int64_t stride, int64_t idx,
                                               double* sh) {
    for (int b = threadIdx.x; b < nb; b += 256) sh[b] = part[(int64_t)b * stride + idx];
    __syncthreads();
    double sum = 0.0;
    if (threadIdx.x == 0)
        for (int b = 0; b < nb; ++b) sum += sh[b];
    __syncthreads();
    return sum;
}

// the largest of part[b * stride + idx], b < nb (thread 0's return)
__device__ __forceinline__ ull max_partials(const ull* __restrict__ part, int nb, int64_t stride, int64_t idx,
                                            ull* sh) {
    ull m = 0;
    for (int b = threadIdx.x; b < nb; b += 256) m = umax(m, part[(int64_t)b * stride + idx]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = umax(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    const ull r = sh[0];
    __syncthreads();
    return r;
}

// what refine_scale_cast reads of a column
__device__ __forceinline__ void mirror(const PcgCol& c, RefineCol& r) {
    r.active = c.active;
    r.scale = c.scale;
}

__global__ __launch_bounds__(256) void pcg_judge_alpha(int nb, int64_t k, const double* __restrict__ part,
                                                       PcgCol* __restrict__ st, RefineCol* __restrict__ rst) {
    __shared__ double sh[REFINE_MAX_BLOCKS];
    for (int64_t j = 0; j < k; ++j) {
        if (!st[j].active) continue;
        const double pq = sum_partials(part, nb, k, j, sh);
        if (threadIdx.x == 0) {
            PcgCol c = st[j];
            pcg_rule_alpha(c, pq);
            st[j] = c;
            mirror(c, rst[j]);
        }
    }
}

__global__ __launch_bounds__(256) void pcg_judge_beta(int nb, int64_t k, const double* __restrict__ part,
                                                      PcgCol* __restrict__ st, RefineCol* __restrict__ rst) {
    __shared__ double sh[REFINE_MAX_BLOCKS];
    for (int64_t j = 0; j < k; ++j) {
        if (!st[j].active) continue;
        const double rz = sum_partials(part, nb, 2 * k, j, sh);
        const double qz = sum_partials(part, nb, 2 * k, k + j, sh);
        if (threadIdx.x == 0) {
            PcgCol c = st[j];
            pcg_rule_beta(c, rz, qz);
            st[j] = c;
            mirror(c, rst[j]);
        }
    }
}

// mode 0: the first iterate (every column), 1: step `it` (the active
// columns), 2: the true residual of the columns that asked, 3: the end (the
// columns without a true residual). part: [block][2][k] maxima of |r|, |x|.
__global__ __launch_bounds__(256) void pcg_judge_norms(int nb, int64_t k, const ull* __restrict__ part, double snorm,
                                                       double tol, int mode, uint32_t it, PcgCol* __restrict__ st,
                                                       RefineCol* __restrict__ rst) {
    __shared__ ull sh[256];
    for (int64_t j = 0; j < k; ++j) {
        if (mode == 1 && !st[j].active) continue;
        if (mode == 2 && !st[j].verify) continue;
        const ull br = max_partials(part, nb, 2 * k, j, sh);
        const ull bx = max_partials(part, nb, 2 * k, k + j, sh);
        if (threadIdx.x == 0) {
            PcgCol c = st[j];
            const double rmax = bits_abs(br), xmax = bits_abs(bx);
            const double bnorm = mode == 0 ? rst[j].bnorm : c.bnorm;
            const double omega = refine_omega(rmax, xmax, bnorm, snorm);
            if (mode == 0) pcg_rule_init(c, bnorm, omega, rmax, tol);
            else if (mode == 1) pcg_rule_step(c, it, omega, rmax, tol);
            else if (mode == 2) pcg_rule_verified(c, omega, rmax, tol);
            else pcg_rule_final(c, omega);
            st[j] = c;
            mirror(c, rst[j]);
        }
    }
}

template <typename TA, int G>
int spmv_launch_g(unsigned nb, int64_t n, int64_t k, const bsm_sym* S, const double* P, double* Q, const PcgCol* st,
                  double* part, hipStream_t s) {
    const TA* v = static_cast<const TA*>(S->vals);
    if (k % 4 == 0) pcg_spmv_dot<TA, G, 4><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, P, Q, st, part);
    else if (k % 2 == 0) pcg_spmv_dot<TA, G, 2><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, P, Q, st, part);
    else pcg_spmv_dot<TA, G, 1><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, P, Q, st, part);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

// G from S's mean row length and the workgroups from n, as refine_resid's
template <typename TA>
int spmv_launch(int64_t n, int64_t k, const bsm_sym* S, const double* P, double* Q, const PcgCol* st, double* part,
                unsigned* nb_out, hipStream_t s) {
    const int g = resid_group(S, n);
    const unsigned nb = resid_blocks(g, n);
    *nb_out = nb;
    switch (g) {
        case 4: return spmv_launch_g<TA, 4>(nb, n, k, S, P, Q, st, part, s);
        case 8: return spmv_launch_g<TA, 8>(nb, n, k, S, P, Q, st, part, s);
        case 16: return spmv_launch_g<TA, 16>(nb, n, k, S, P, Q, st, part, s);
        default: return spmv_launch_g<TA, 64>(nb, n, k, S, P, Q, st, part, s);
    }
}

template <typename TF>
int dots_launch(unsigned nb, int64_t n, int64_t k, const TF* W, const double* R, const double* Q, const PcgCol* st,
                double* part, hipStream_t s) {
    if (k % 4 == 0) pcg_dots<TF, 4><<<nb, 256, 0, s>>>(n, k, W, R, Q, st, part);
    else if (k % 2 == 0) pcg_dots<TF, 2><<<nb, 256, 0, s>>>(n, k, W, R, Q, st, part);
    else pcg_dots<TF, 1><<<nb, 256, 0, s>>>(n, k, W, R, Q, st, part);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

int step_launch(unsigned nb, int64_t n, int64_t k, const double* P, const double* Q, double* X, double* R,
                const PcgCol* st, ull* part, hipStream_t s) {
    if (k % 4 == 0) pcg_step_xr<4><<<nb, 256, 0, s>>>(n, k, P, Q, X, R, st, part);
    else if (k % 2 == 0) pcg_step_xr<2><<<nb, 256, 0, s>>>(n, k, P, Q, X, R, st, part);
    else pcg_step_xr<1><<<nb, 256, 0, s>>>(n, k, P, Q, X, R, st, part);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

template <typename TA, typename TF>
int pcg_t(const bsm_nd_factor* f, const bsm_csr* a, const bsm_sym* S, int64_t n, int64_t k, const void* b_dev,
          void* x_dev, uint32_t max_iter, double tol, std::vector<PcgCol>& cols, hipStream_t s) {
    const size_t nk = (size_t)n * (size_t)k;
    const unsigned eb = (unsigned)((nk + 255) / 256);
    const unsigned vb = pcg_blocks((uint64_t)n, 256);  // the row-per-thread kernels: a function of n alone
    DBuf Bb, Xb, Rb, Rtb, Pb, Qb, Wb, partb, dpartb, stb, rstb;
    DrainOnError drain{s};
    BSM_TRY(Bb.alloc(nk * sizeof(double), s));
    BSM_TRY(Xb.alloc(nk * sizeof(double), s));
    BSM_TRY(Rb.alloc(nk * sizeof(double), s));
    BSM_TRY(Rtb.alloc(nk * sizeof(double), s));
    BSM_TRY(Pb.alloc(nk * sizeof(double), s));
    BSM_TRY(Qb.alloc(nk * sizeof(double), s));
    BSM_TRY(Wb.alloc(nk * sizeof(TF), s));
    BSM_TRY(partb.alloc((size_t)REFINE_MAX_BLOCKS * 2 * (size_t)k * sizeof(ull), s));
    BSM_TRY(dpartb.alloc((size_t)REFINE_MAX_BLOCKS * 2 * (size_t)k * sizeof(double), s));
    BSM_TRY(stb.alloc((size_t)k * sizeof(PcgCol), s));
    BSM_TRY(rstb.alloc((size_t)k * sizeof(RefineCol), s));
    double *B = Bb.as<double>(), *X = Xb.as<double>(), *R = Rb.as<double>(), *Rt = Rtb.as<double>();
    double *P = Pb.as<double>(), *Q = Qb.as<double>(), *dpart = dpartb.as<double>();
    TF* W = Wb.as<TF>();
    ull* part = partb.as<ull>();
    PcgCol* st = stb.as<PcgCol>();
    RefineCol* rst = rstb.as<RefineCol>();
    auto any_of = [&](auto pred) {
        bool any = false;
        for (const PcgCol& c : cols) any = any || pred(c);
        return any;
    };

    // p and q are read before they are written only where beta = 0 / the dots are unused
    BSM_HIP_TRY(hipMemsetAsync(P, 0, nk * sizeof(double), s));
    BSM_HIP_TRY(hipMemsetAsync(Q, 0, nk * sizeof(double), s));
    unsigned nb = 0;
    BSM_TRY(refine_first_iterate(f, a, S, n, k, b_dev, B, X, R, W, part, rst, &nb, s));
    pcg_judge_norms<<<1, 256, 0, s>>>((int)nb, k, part, S->norm_inf, tol, 0, 0, st, rst);
    BSM_HIP_TRY(hipGetLastError());
    BSM_HIP_TRY(read_dev(cols.data(), st, (size_t)k * sizeof(PcgCol), s));
    for (uint32_t it = 1; it <= max_iter && any_of([](const PcgCol& c) { return c.active != 0; }); ++it) {
        BSM_TRY(refine_precondition(f, n, k, R, rst, W, s));  // all k columns; the stopped ones carry zeros
        BSM_TRY(dots_launch<TF>(vb, n, k, W, R, Q, st, dpart, s));
        pcg_judge_beta<<<1, 256, 0, s>>>((int)vb, k, dpart, st, rst);
        BSM_HIP_TRY(hipGetLastError());
        pcg_update_p<TF><<<eb, 256, 0, s>>>(n, k, W, st, P);
        BSM_HIP_TRY(hipGetLastError());
        stage_mark("pcg_dots_p", s);  // the stage list is the last solve's, then these (bsm_stage_times)
        BSM_TRY(spmv_launch<TA>(n, k, S, P, Q, st, dpart, &nb, s));
        pcg_judge_alpha<<<1, 256, 0, s>>>((int)nb, k, dpart, st, rst);
        BSM_HIP_TRY(hipGetLastError());
        stage_mark("pcg_spmv_dot", s);
        BSM_TRY(step_launch(vb, n, k, P, Q, X, R, st, part, s));
        pcg_judge_norms<<<1, 256, 0, s>>>((int)vb, k, part, S->norm_inf, tol, 1, it, st, rst);
        BSM_HIP_TRY(hipGetLastError());
        stage_mark("pcg_step_xr", s);
        BSM_HIP_TRY(read_dev(cols.data(), st, (size_t)k * sizeof(PcgCol), s));
        if (any_of([](const PcgCol& c) { return c.verify != 0; })) {
            // the true residual of every column; only the asking ones take it
            BSM_TRY(refine_residual(a, S, n, k, X, B, Rt, part, &nb, s));
            pcg_judge_norms<<<1, 256, 0, s>>>((int)nb, k, part, S->norm_inf, tol, 2, it, st, rst);
            BSM_HIP_TRY(hipGetLastError());
            pcg_take_r<<<eb, 256, 0, s>>>(n, k, Rt, st, R);
            BSM_HIP_TRY(hipGetLastError());
            stage_mark("pcg_verify", s);
            BSM_HIP_TRY(read_dev(cols.data(), st, (size_t)k * sizeof(PcgCol), s));
        }
    }
    if (any_of([](const PcgCol& c) { return !c.zero && !c.verified; })) {
        BSM_TRY(refine_residual(a, S, n, k, X, B, Rt, part, &nb, s));
        pcg_judge_norms<<<1, 256, 0, s>>>((int)nb, k, part, S->norm_inf, tol, 3, 0, st, rst);
        BSM_HIP_TRY(hipGetLastError());
        BSM_HIP_TRY(read_dev(cols.data(), st, (size_t)k * sizeof(PcgCol), s));
    }
    pcg_finish<TA><<<eb, 256, 0, s>>>(n, k, X, st, static_cast<TA*>(x_dev));
    BSM_HIP_TRY(hipGetLastError());
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    return BSM_OK;
}

}  // namespace

int nd_pcg_solve(const bsm_nd_factor* f, const bsm_csr* a, uint64_t k, const void* b_dev, void* x_dev,
                 uint32_t max_iter, double tol, uint32_t* iters, double* berr, uint32_t* flags, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(f->mu);
        BSM_REQUIRE(f->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first");
    }
    const int64_t n = (int64_t)f->n;
    std::vector<PcgCol> cols((size_t)k);
    if (n > 0 && k > 0) {
        BSM_REQUIRE(k < ((uint64_t)1 << 31), BSM_ERR_UNSUPPORTED, "pcg solve: k >= 2^31");
        const bsm_sym* S = nullptr;
        BSM_TRY(sym_obtain(a, s, &S));
        if (tol == 0.0) tol = refine_default_tol(S->max_len);
        int rc;
        if (a->dtype == BSM_F64)
            rc = f->dtype == BSM_F64 ? pcg_t<double, double>(f, a, S, n, (int64_t)k, b_dev, x_dev, max_iter, tol, cols, s)
                                     : pcg_t<double, float>(f, a, S, n, (int64_t)k, b_dev, x_dev, max_iter, tol, cols, s);
        else
            rc = f->dtype == BSM_F64 ? pcg_t<float, double>(f, a, S, n, (int64_t)k, b_dev, x_dev, max_iter, tol, cols, s)
                                     : pcg_t<float, float>(f, a, S, n, (int64_t)k, b_dev, x_dev, max_iter, tol, cols, s);
        BSM_TRY(rc);
    }
    for (uint64_t j = 0; j < k; ++j) {
        if (iters) iters[j] = cols[j].iters;
        if (berr) berr[j] = cols[j].omega;
        if (flags) flags[j] = cols[j].breakdown ? 1u : 0u;
    }
    return BSM_OK;
}

}  // namespace bsm
