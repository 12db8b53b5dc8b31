// kernels_eig.hip -- the smallest eigenpairs of S by block shift-invert
// Lanczos on a kept nd factor (bsm_nd_factor_eigsh, gfx950). S is a's lower
// triangle mirrored (sym_obtain), the operator is A^-1 by the refined solve
// (nd_refine_solve: f64 backward error whichever dtype the factor has), the
// basis V_0, V_1, ... is kept as n x p row-major f64 blocks, and a step is
//   W = A^-1 V_j                               eig_cast, nd_refine_solve
//   C = V^T W, W -= V C, twice                 eig_vtw, eig_sum, eig_combine<SUB>
//   G = W^T W = R1^T R1, W = W R1^-1, again    eig_judge, eig_combine<MUL>
//   A_j, B_{j+1} = R2 R1 into T; T s = theta s  the host, eig_rule.hpp
// and the end is Y = V Z (eig_combine<YVZ>) with the true residuals S Y - Y
// diag(lambda) (eig_resid, refine_resid's lane layout).
// A workgroup owns a row range that depends on n and p alone and walks it in
// tiles kept in LDS: a tile of V_b and of W are loaded with contiguous reads,
// then thread (c, d) adds the tile's rows of V[., c] W[., d] in row order.
// The per-workgroup partials are added in index order by one workgroup; there
// are no floating-point atomics, so the same call gives the same bits. One
// reorthogonalisation step reads V twice per pass: about 4 n m 8 bytes for m
// basis columns. The generalised problem S y = lambda S_M y
// (bsm_nd_factor_eigsh_gen) is the same loop in the S_M inner product, with
// kernels and a host loop of its own below (eigsh_gen_t); eigsh_t is not
// touched by it.
#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "bsm_internal.hpp"
#include "eig_rule.hpp"

namespace bsm {
namespace {

constexpr int EIG_TILE = 2048;  // f64 values of a tile: tr rows of p columns

// rows of a tile, the workgroups and the rows of one: functions of n and p alone
struct EigGeom {
    int tr = 0;
    unsigned nb = 0;
    int64_t rw = 0;
};

EigGeom eig_geom(int64_t n, int p) {
    EigGeom g;
    g.tr = std::min(256, EIG_TILE / p);
    const int64_t tiles = (n + g.tr - 1) / g.tr;
    const int64_t nb0 = std::max<int64_t>(1, std::min<int64_t>(tiles, REFINE_MAX_BLOCKS));
    g.rw = (tiles + nb0 - 1) / nb0 * g.tr;
    g.nb = (unsigned)std::max<int64_t>(1, (n + g.rw - 1) / g.rw);
    return g;
}

// the start block: hash values in [-1, 1), rounded to a's dtype (so that a
// caller's v0 of that dtype can restate them)
template <typename TA>
__global__ __launch_bounds__(256) void eig_fill(int64_t n, int64_t p, uint64_t seed, double* __restrict__ W) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * p) return;
    W[i] = (double)(TA)eig_start_value(seed, (uint64_t)(i / p), (uint64_t)(i % p));
}

template <typename TD, typename TS>
__global__ __launch_bounds__(256) void eig_cast(int64_t cnt, const TS* __restrict__ src, TD* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cnt) dst[i] = (TD)src[i];
}

// out[row][c0 + c] = Y[row][c], c < cols: a chunk of the vectors into the n x nev result
template <typename TA>
__global__ __launch_bounds__(256) void eig_store_cols(int64_t n, int64_t p, int64_t nev, int64_t c0, int64_t cols,
                                                      const double* __restrict__ Y, TA* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * cols) return;
    const int64_t row = i / cols, c = i % cols;
    out[row * nev + c0 + c] = (TA)Y[row * p + c];
}

// tile[i] = src[i] for i < have, 0 up to cnt
__device__ __forceinline__ void load_tile(double* tile, const double* __restrict__ src, int have, int cnt) {
    for (int i = threadIdx.x; i < cnt; i += 256) tile[i] = i < have ? src[i] : 0.0;
}

// acc[i] += sum over the tile's tr rows of At[r][c] Bt[r][d] for the entry
// e = tid + 256 i = c p + d. Up to 128 entries: 256 / E slices of rows, each
// added in row order, then the slices in slice order (red: 256 values).
__device__ __forceinline__ void tile_products(int p, int tr, const double* At, const double* Bt, double* red,
                                              double (&acc)[4]) {
    const int E = p * p;
    if (E <= 128) {
        const int ns = 256 / E, rs = (tr + ns - 1) / ns;
        const int e = threadIdx.x % E, sl = threadIdx.x / E;
        if (sl < ns) {
            const int c = e / p, d = e % p;
            double sum = 0.0;
            const int r1 = min(tr, (sl + 1) * rs);
            for (int r = sl * rs; r < r1; ++r) sum = fma(At[r * p + c], Bt[r * p + d], sum);
            red[sl * E + e] = sum;
        }
        __syncthreads();
        if (sl == 0) {
            double sum = 0.0;
            for (int q = 0; q < ns; ++q) sum += red[q * E + e];
            acc[0] += sum;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + 256 * i;
            if (e < E) {
                const int c = e / p, d = e % p;
                double sum = 0.0;
                for (int r = 0; r < tr; ++r) sum = fma(At[r * p + c], Bt[r * p + d], sum);
                acc[i] += sum;
            }
        }
    }
    __syncthreads();
}

// part[block][b][c][d] = the workgroup's share of V_b[., c] . W[., d], for
// the nblk basis blocks and, with_w, for W itself as one more (W^T W)
__global__ __launch_bounds__(256) void eig_vtw(int64_t n, int p, int tr, int64_t rw, int nblk, int with_w,
                                               const double* __restrict__ V, const double* __restrict__ W,
                                               double* __restrict__ part) {
    __shared__ double At[EIG_TILE], Bt[EIG_TILE], red[256];
    const int E = p * p, nall = nblk + with_w;
    const int64_t lo = (int64_t)blockIdx.x * rw, hi = min(n, lo + rw);
    for (int b = 0; b < nall; ++b) {
        const double* src = b < nblk ? V + (int64_t)b * n * p : W;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t t0 = lo; t0 < hi; t0 += tr) {
            const int have = (int)min((int64_t)tr, hi - t0) * p;
            load_tile(At, src + t0 * p, have, tr * p);
            load_tile(Bt, W + t0 * p, have, tr * p);
            __syncthreads();
            tile_products(p, tr, At, Bt, red, acc);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + 256 * i;
            if (e < E) part[((int64_t)blockIdx.x * nall + b) * E + e] = acc[i];
        }
    }
}

// out[e] = the sum of part[b][e], b < nb, in index order (one workgroup).
// Entry e of basis block jblk also goes into rec (pass 1) or is added to it
// (pass 2): the summed projections onto V_j; the diagonal of block wblk (W^T
// W) is norm2, the columns' squared norms before the projections.
__global__ __launch_bounds__(256) void eig_sum(int nb, int cnt, const double* __restrict__ part,
                                               double* __restrict__ out, int p, int jblk, int wblk, int pass,
                                               double* __restrict__ rec, double* __restrict__ norm2) {
    const int E = p * p;
    for (int e = threadIdx.x; e < cnt; e += 256) {
        double sum = 0.0;
        for (int b = 0; b < nb; ++b) sum += part[(int64_t)b * cnt + e];
        out[e] = sum;
        const int blk = e / E, idx = e % E;
        if (blk == jblk) rec[idx] = pass == 1 ? sum : rec[idx] + sum;
        if (blk == wblk && idx / p == idx % p) norm2[idx / p] = sum;
    }
}

enum { EIG_SUB = 0, EIG_MUL = 1, EIG_YVZ = 2, EIG_SUBP = 3 };

// SUB: out = W - sum_b V_b M_b (M = C, m x p), the projections taken off in
//      basis order; MUL: out = W M (M = U, p x p); YVZ: out = sum_b V_b M_b
//      (M = Z, m x p). SUB and MUL also give gpart[block][c][d], the
//      workgroup's share of out^T out. SUBP is SUB without that Gram matrix
//      (the generalised problem's is out^T S_M out). out may be W.
template <int MODE>
__global__ __launch_bounds__(256) void eig_combine(int64_t n, int p, int tr, int64_t rw, int nblk,
                                                   const double* __restrict__ V, const double* W,
                                                   const double* __restrict__ M, double* out,
                                                   double* __restrict__ gpart) {
    __shared__ double At[EIG_TILE], Bt[EIG_TILE], red[256];
    constexpr bool TAKE_OFF = MODE == EIG_SUB || MODE == EIG_SUBP, GRAM = MODE == EIG_SUB || MODE == EIG_MUL;
    const int E = p * p;
    const int64_t lo = (int64_t)blockIdx.x * rw, hi = min(n, lo + rw);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t0 = lo; t0 < hi; t0 += tr) {
        const int have = (int)min((int64_t)tr, hi - t0) * p;
        double w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = threadIdx.x + 256 * u;
            w[u] = (TAKE_OFF && i < have) ? W[t0 * p + i] : 0.0;
        }
        if constexpr (MODE == EIG_MUL) {
            load_tile(At, W + t0 * p, have, tr * p);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = threadIdx.x + 256 * u;
                if (i < have) {
                    const int r = i / p, d = i % p;
                    for (int c = 0; c < p; ++c) w[u] = fma(At[r * p + c], M[c * p + d], w[u]);
                }
            }
            __syncthreads();
        } else {
            for (int b = 0; b < nblk; ++b) {
                load_tile(At, V + ((int64_t)b * n + t0) * p, have, tr * p);
                __syncthreads();
                const double* Mb = M + (int64_t)b * E;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = threadIdx.x + 256 * u;
                    if (i < have) {
                        const int r = i / p, d = i % p;
                        for (int c = 0; c < p; ++c) {
                            const double v = At[r * p + c];
                            w[u] = fma(TAKE_OFF ? -v : v, Mb[c * p + d], w[u]);
                        }
                    }
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = threadIdx.x + 256 * u;
            if (i < have) out[t0 * p + i] = w[u];
            if (GRAM && i < tr * p) Bt[i] = i < have ? w[u] : 0.0;
        }
        if constexpr (GRAM) {
            __syncthreads();
            tile_products(p, tr, Bt, Bt, red, acc);
        }
    }
    if constexpr (GRAM) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + 256 * i;
            if (e < E) gpart[(int64_t)blockIdx.x * E + e] = acc[i];
        }
    }
}

// The step's record, which the host reads once: [0, E) the summed projections
// onto V_j, [E, 2E) R1, [2E, 3E) R2, [3E, 4E) the Gram matrix the first
// Cholesky got, [4E] 1 while the block has full rank.
// One workgroup: G = the Gram partials in index order, its Cholesky with the
// rank rule (eig_rule.hpp; which == 1 only), U = R^-1 for the next eig_combine.
__global__ __launch_bounds__(256) void eig_judge(int nb, int p, const double* __restrict__ gpart,
                                                 const double* __restrict__ norm2, int which,
                                                 double* __restrict__ rec, double* __restrict__ U) {
    __shared__ double G[1024], R[1024], Us[1024];
    __shared__ int ok;
    const int E = p * p;
    for (int e = threadIdx.x; e < E; e += 256) {
        double sum = 0.0;
        for (int b = 0; b < nb; ++b) sum += gpart[(int64_t)b * E + e];
        G[e] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) ok = eig_chol_rank(p, G, which == 1 ? norm2 : nullptr, R, Us);
    __syncthreads();
    for (int e = threadIdx.x; e < E; e += 256) {
        rec[which * E + e] = R[e];
        U[e] = Us[e];
        if (which == 1) rec[3 * E + e] = G[e];
    }
    if (threadIdx.x == 0) {
        if (which == 1) rec[4 * E] = ok ? 1.0 : 0.0;
        else if (!ok) rec[4 * E] = 0.0;
    }
}

// part[block][0][j] = the workgroup's share of ||r_j||^2, part[block][1][j] of
// ||y_j||^2, r = S y - lambda y: refine_resid's lane layout (G lanes per row
// take the row's entries in stored order, explicit fma, a fixed xor tree); a
// group's lane 0 adds its rows in row order, the groups are added in order.
template <typename TA, int G, int KC>
__global__ __launch_bounds__(256) void eig_resid(int64_t n, int64_t k, const int64_t* __restrict__ rp,
                                                 const int32_t* __restrict__ col, const TA* __restrict__ val,
                                                 const double* __restrict__ Y, const double* __restrict__ lam,
                                                 double* __restrict__ part) {
    constexpr int GROUPS = 256 / G;
    __shared__ double sh[GROUPS][2 * KC];
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    for (int64_t j0 = 0; j0 < k; j0 += KC) {
        double rr[KC], yy[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) rr[c] = yy[c] = 0.0;
        for (int64_t row0 = (int64_t)blockIdx.x * GROUPS; row0 < n; row0 += (int64_t)gridDim.x * GROUPS) {
            const int64_t row = row0 + grp;
            double acc[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) acc[c] = 0.0;
            if (row < n) {
                const int64_t e1 = rp[row + 1];
                for (int64_t e = rp[row] + lane; e < e1; e += G) {
                    const double v = (double)val[e];
                    const double* yp = Y + (int64_t)col[e] * k + j0;
#pragma unroll
                    for (int c = 0; c < KC; ++c) acc[c] = fma(v, yp[c], acc[c]);
                }
            }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
#pragma unroll
                for (int c = 0; c < KC; ++c) acc[c] += __shfl_xor(acc[c], o);
            }
            if (lane == 0 && row < n) {
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const double y = Y[row * k + j0 + c];
                    const double r = fma(-lam[j0 + c], y, acc[c]);
                    rr[c] = fma(r, r, rr[c]);
                    yy[c] = fma(y, y, yy[c]);
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                sh[grp][c] = rr[c];
                sh[grp][KC + c] = yy[c];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * KC) {
            double sum = 0.0;
            for (int g = 0; g < GROUPS; ++g) sum += sh[g][threadIdx.x];
            const int which = threadIdx.x / KC, c = threadIdx.x % KC;
            part[((int64_t)blockIdx.x * 2 + which) * k + j0 + c] = sum;
        }
        __syncthreads();
    }
}

template <typename TA, int G>
int eig_resid_g(unsigned nb, int64_t n, int64_t k, const bsm_sym* S, const double* Y, const double* lam, double* part,
                hipStream_t s) {
    const TA* v = static_cast<const TA*>(S->vals);
    if (k % 4 == 0) eig_resid<TA, G, 4><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, Y, lam, part);
    else if (k % 2 == 0) eig_resid<TA, G, 2><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, Y, lam, part);
    else eig_resid<TA, G, 1><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, Y, lam, part);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

// G from S's mean row length and the workgroups from n, as refine_resid's
template <typename TA>
int eig_resid_launch(int64_t n, int64_t k, const bsm_sym* S, const double* Y, const double* lam, double* part,
                     unsigned* nb_out, hipStream_t s) {
    const int g = resid_group(S, n);
    const unsigned nb = resid_blocks(g, n);
    *nb_out = nb;
    switch (g) {
        case 4: return eig_resid_g<TA, 4>(nb, n, k, S, Y, lam, part, s);
        case 8: return eig_resid_g<TA, 8>(nb, n, k, S, Y, lam, part, s);
        case 16: return eig_resid_g<TA, 16>(nb, n, k, S, Y, lam, part, s);
        default: return eig_resid_g<TA, 64>(nb, n, k, S, Y, lam, part, s);
    }
}

int upload(void* dst, const void* src, size_t bytes, hipStream_t s) {
    BSM_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    BSM_HIP_TRY(hipStreamSynchronize(s));  // src is pageable and the caller's to change
    return BSM_OK;
}

struct EigOut {
    std::vector<double> lam, resid;
    uint32_t info[4] = {0, 0, 0, 0};
};

template <typename TA>
int eigsh_t(const bsm_nd_factor* f, const bsm_csr* a, const bsm_sym* S, int64_t n, int nev, int p, int ncv, double tol,
            uint64_t seed, const void* v0_dev, void* vec_dev, EigOut& res, hipStream_t s) {
    const int E = p * p;
    const size_t np = (size_t)n * (size_t)p;
    const unsigned eb = (unsigned)((np + 255) / 256);
    const EigGeom g = eig_geom(n, p);
    const int maxblk = ncv / p;
    DBuf Vb, Wb, Tb, Yb, partb, gpartb, Cb, recb, Ub, n2b, lamb, sumb;
    DrainOnError drain{s};
    BSM_TRY(Vb.alloc((size_t)ncv * (size_t)n * sizeof(double), s));
    BSM_TRY(Wb.alloc(np * sizeof(double), s));
    BSM_TRY(Tb.alloc(np * sizeof(double), s));
    BSM_TRY(Yb.alloc(np * sizeof(double), s));
    BSM_TRY(partb.alloc(std::max((size_t)g.nb * (size_t)(maxblk + 1) * E, (size_t)REFINE_MAX_BLOCKS * 2 * p) *
                            sizeof(double), s));
    BSM_TRY(gpartb.alloc((size_t)g.nb * E * sizeof(double), s));
    BSM_TRY(Cb.alloc((size_t)(maxblk + 1) * E * sizeof(double), s));
    BSM_TRY(recb.alloc((size_t)(4 * E + 1) * sizeof(double), s));
    BSM_TRY(Ub.alloc((size_t)E * sizeof(double), s));
    BSM_TRY(n2b.alloc((size_t)p * sizeof(double), s));
    BSM_TRY(lamb.alloc((size_t)p * sizeof(double), s));
    BSM_TRY(sumb.alloc((size_t)2 * p * sizeof(double), s));
    double *V = Vb.as<double>(), *W = Wb.as<double>(), *Y = Yb.as<double>(), *part = partb.as<double>();
    double *gpart = gpartb.as<double>(), *C = Cb.as<double>(), *rec = recb.as<double>(), *U = Ub.as<double>();
    double *norm2 = n2b.as<double>(), *lamd = lamb.as<double>(), *sums = sumb.as<double>();
    TA* T = Tb.as<TA>();
    std::vector<double> h((size_t)4 * E + 1), B((size_t)E);
    uint32_t flags = 0;

    // C = [V_0 .. V_{nblk-1} (W)]^T W into C, the record and norm2
    auto project = [&](int nblk, int with_w, int pass) -> int {
        const int nall = nblk + with_w;
        eig_vtw<<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, nblk, with_w, V, W, part);
        BSM_HIP_TRY(hipGetLastError());
        eig_sum<<<1, 256, 0, s>>>((int)g.nb, nall * E, part, C, p, nblk - 1, with_w ? nblk : -1, pass, rec, norm2);
        BSM_HIP_TRY(hipGetLastError());
        return BSM_OK;
    };
    // Cholesky-QR twice on W, from the Gram partials in gp; the result into `to`
    auto orthonormalise = [&](const double* gp, double* to) -> int {
        eig_judge<<<1, 256, 0, s>>>((int)g.nb, p, gp, norm2, 1, rec, U);
        BSM_HIP_TRY(hipGetLastError());
        eig_combine<EIG_MUL><<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, 0, nullptr, W, U, W, gpart);
        BSM_HIP_TRY(hipGetLastError());
        eig_judge<<<1, 256, 0, s>>>((int)g.nb, p, gpart, nullptr, 2, rec, U);
        BSM_HIP_TRY(hipGetLastError());
        eig_combine<EIG_MUL><<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, 0, nullptr, W, U, to, gpart);
        BSM_HIP_TRY(hipGetLastError());
        return read_dev(h.data(), rec, h.size() * sizeof(double), s) == hipSuccess ? BSM_OK : BSM_ERR_HIP;
    };

    EigLoop loop;
    loop.init(p, nev, ncv, tol);
    if (v0_dev) eig_cast<double, TA><<<eb, 256, 0, s>>>((int64_t)np, static_cast<const TA*>(v0_dev), W);
    else eig_fill<TA><<<eb, 256, 0, s>>>(n, p, seed, W);
    BSM_HIP_TRY(hipGetLastError());
    BSM_TRY(project(0, 1, 1));  // W^T W: the Gram partials, and norm2
    if (orthonormalise(part, V) != BSM_OK) {
        set_error("eigsh: reading the step's record failed");
        return BSM_ERR_HIP;
    }
    bool have_basis = h[(size_t)4 * E] != 0.0;
    if (!have_basis) flags |= EIG_EXHAUSTED;  // a start block without full rank spans nothing to iterate on
    stage_mark("eig_qr", s);

    const double rtol = refine_default_tol(S->max_len);
    std::vector<uint32_t> it((size_t)p);
    std::vector<double> be((size_t)p);
    while (have_basis) {
        const int j = loop.steps, nblk = j + 1;
        const double* Vj = V + (size_t)j * np;
        eig_cast<TA, double><<<eb, 256, 0, s>>>((int64_t)np, Vj, T);
        BSM_HIP_TRY(hipGetLastError());
        BSM_TRY(nd_refine_solve(f, a, (uint64_t)p, T, T, 5, 0.0, it.data(), be.data(), s));
        eig_cast<double, TA><<<eb, 256, 0, s>>>((int64_t)np, T, W);
        BSM_HIP_TRY(hipGetLastError());
        stage_mark("eig_solve", s);  // the stage list is the last solve's, then these (bsm_stage_times)
        for (double e : be)
            if (!(e <= rtol)) flags |= EIG_INEXACT;
        for (int pass = 1; pass <= 2; ++pass) {
            BSM_TRY(project(nblk, pass == 1, pass));
            eig_combine<EIG_SUB><<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, nblk, V, W, C, W, gpart);
            BSM_HIP_TRY(hipGetLastError());
        }
        stage_mark("eig_reorth", s);
        const bool room = (nblk + 1) * p <= ncv;
        if (orthonormalise(gpart, room ? V + (size_t)nblk * np : W) != BSM_OK) {
            set_error("eigsh: reading the step's record failed");
            return BSM_ERR_HIP;
        }
        stage_mark("eig_qr", s);
        const bool full = h[(size_t)4 * E] != 0.0;
        if (full) eig_mul_upper(p, &h[(size_t)2 * E], &h[(size_t)E], B.data());
        loop.push(h.data(), full ? B.data() : nullptr);
        if (!full) {
            flags |= EIG_EXHAUSTED;
            loop.ritz(&h[(size_t)3 * E]);
            stage_mark("eig_ritz", s);
            break;
        }
        if (loop.check_due(loop.steps)) {
            loop.ritz();
            stage_mark("eig_ritz", s);  // the stream is idle meanwhile: the host's time
            if (loop.done()) break;
        }
        if (!room) break;
    }
    if (have_basis && loop.m_ritz != loop.m()) loop.ritz();

    // the wanted pairs, lambda ascending
    const int m = loop.m(), got = std::min(nev, m);
    std::vector<int> order((size_t)got);
    std::iota(order.begin(), order.end(), 0);
    std::vector<double> lam_all((size_t)got);
    for (int i = 0; i < got; ++i) lam_all[(size_t)i] = 1.0 / loop.theta_of(i);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lam_all[(size_t)x] < lam_all[(size_t)y]; });
    const double nan = std::numeric_limits<double>::quiet_NaN();
    res.lam.assign((size_t)nev, nan);
    res.resid.assign((size_t)nev, nan);
    if (vec_dev && got < nev) BSM_HIP_TRY(hipMemsetAsync(vec_dev, 0, (size_t)n * (size_t)nev * sizeof(TA), s));
    std::vector<double> Z((size_t)m * p), lamc((size_t)p), sum_h((size_t)2 * p);
    for (int c0 = 0; c0 < got; c0 += p) {
        const int cols = std::min(p, got - c0);
        std::fill(Z.begin(), Z.end(), 0.0);
        std::fill(lamc.begin(), lamc.end(), 0.0);
        for (int c = 0; c < cols; ++c) {
            const int i = order[(size_t)(c0 + c)];
            lamc[(size_t)c] = lam_all[(size_t)i];
            for (int r = 0; r < m; ++r) Z[(size_t)r * p + c] = loop.s_of(i, r);
        }
        BSM_TRY(upload(C, Z.data(), Z.size() * sizeof(double), s));  // C holds (ncv + p) p values
        BSM_TRY(upload(lamd, lamc.data(), lamc.size() * sizeof(double), s));
        eig_combine<EIG_YVZ><<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, m / p, V, nullptr, C, Y, nullptr);
        BSM_HIP_TRY(hipGetLastError());
        if constexpr (sizeof(TA) < sizeof(double)) {  // the residual is that of the vectors as they are returned
            eig_cast<TA, double><<<eb, 256, 0, s>>>((int64_t)np, Y, T);
            BSM_HIP_TRY(hipGetLastError());
            eig_cast<double, TA><<<eb, 256, 0, s>>>((int64_t)np, T, Y);
            BSM_HIP_TRY(hipGetLastError());
        }
        unsigned nb = 0;
        BSM_TRY(eig_resid_launch<TA>(n, p, S, Y, lamd, part, &nb, s));
        eig_sum<<<1, 256, 0, s>>>((int)nb, 2 * p, part, sums, p, -1, -1, 0, nullptr, nullptr);
        BSM_HIP_TRY(hipGetLastError());
        BSM_HIP_TRY(read_dev(sum_h.data(), sums, sum_h.size() * sizeof(double), s));
        for (int c = 0; c < cols; ++c) {
            res.lam[(size_t)(c0 + c)] = lamc[(size_t)c];
            res.resid[(size_t)(c0 + c)] = std::sqrt(sum_h[(size_t)c]) / std::sqrt(sum_h[(size_t)(p + c)]);
        }
        if (vec_dev) {
            const unsigned sb = (unsigned)(((size_t)n * cols + 255) / 256);
            eig_store_cols<TA><<<sb, 256, 0, s>>>(n, p, nev, c0, cols, Y, static_cast<TA*>(vec_dev));
            BSM_HIP_TRY(hipGetLastError());
        }
    }
    stage_mark("eig_resid", s);
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    res.info[0] = (uint32_t)loop.steps;
    res.info[1] = (uint32_t)m;
    res.info[2] = have_basis ? (uint32_t)loop.converged() : 0u;
    res.info[3] = flags;
    return BSM_OK;
}

// ---- the generalised problem S y = lambda S_M y (bsm_nd_factor_eigsh_gen) ------
// The same loop in the S_M inner product: the operator A^-1 S_M is self-adjoint
// in it, the basis is S_M-orthonormal, and Q = S_M W travels beside W:
//   W = A^-1 (S_M V_j)                        eig_cast, nd_refine_solve
//   Q = S_M W                                 eig_mass
//   C = V^T Q, W -= V C; Q = S_M W; twice     eig_vtu, eig_sum, eig_combine<SUBP>, eig_mass
//   G = W^T Q = R1^T R1, (W, Q) = (W, Q) R1^-1, again    eig_vtu, eig_judge, eig_mul2
// The pass that ends the step leaves V_{j+1} and S_M V_{j+1}: three products
// with S_M per step and one for the start block. T, the Ritz solve and the
// stop rule are eigsh's (EigLoop).

// U = S_M X, X and U n x p row-major f64: eig_resid's lane layout (G lanes per
// row take the row's entries in stored order, explicit fma, a fixed xor tree)
template <typename TA, int G, int KC>
__global__ __launch_bounds__(256) void eig_mass(int64_t n, int64_t p, const int64_t* __restrict__ rp,
                                                const int32_t* __restrict__ col, const TA* __restrict__ val,
                                                const double* __restrict__ X, double* __restrict__ U) {
    constexpr int GROUPS = 256 / G;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    for (int64_t j0 = 0; j0 < p; j0 += KC) {
        for (int64_t row0 = (int64_t)blockIdx.x * GROUPS; row0 < n; row0 += (int64_t)gridDim.x * GROUPS) {
            const int64_t row = row0 + grp;
            double acc[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) acc[c] = 0.0;
            if (row < n) {
                const int64_t e1 = rp[row + 1];
                for (int64_t e = rp[row] + lane; e < e1; e += G) {
                    const double v = (double)val[e];
                    const double* xp = X + (int64_t)col[e] * p + j0;
#pragma unroll
                    for (int c = 0; c < KC; ++c) acc[c] = fma(v, xp[c], acc[c]);
                }
            }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
#pragma unroll
                for (int c = 0; c < KC; ++c) acc[c] += __shfl_xor(acc[c], o);
            }
            if (lane == 0 && row < n) {
#pragma unroll
                for (int c = 0; c < KC; ++c) U[row * p + j0 + c] = acc[c];
            }
        }
    }
}

template <typename TA, int G>
int eig_mass_g(unsigned nb, int64_t n, int64_t p, const bsm_sym* SM, const double* X, double* U, hipStream_t s) {
    const TA* v = static_cast<const TA*>(SM->vals);
    if (p % 4 == 0) eig_mass<TA, G, 4><<<nb, 256, 0, s>>>(n, p, SM->rp, SM->col, v, X, U);
    else if (p % 2 == 0) eig_mass<TA, G, 2><<<nb, 256, 0, s>>>(n, p, SM->rp, SM->col, v, X, U);
    else eig_mass<TA, G, 1><<<nb, 256, 0, s>>>(n, p, SM->rp, SM->col, v, X, U);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

// G from S_M's mean row length and the workgroups from n, as refine_resid's
template <typename TA>
int eig_mass_launch(int64_t n, int64_t p, const bsm_sym* SM, const double* X, double* U, hipStream_t s) {
    const int g = resid_group(SM, n);
    const unsigned nb = resid_blocks(g, n);
    switch (g) {
        case 4: return eig_mass_g<TA, 4>(nb, n, p, SM, X, U, s);
        case 8: return eig_mass_g<TA, 8>(nb, n, p, SM, X, U, s);
        case 16: return eig_mass_g<TA, 16>(nb, n, p, SM, X, U, s);
        default: return eig_mass_g<TA, 64>(nb, n, p, SM, X, U, s);
    }
}

// eig_vtw with the second operand apart from the first:
// part[block][b][c][d] = the workgroup's share of V_b[., c] . U[., d], for the
// nblk basis blocks and, with_w, for W as one more (W^T U)
__global__ __launch_bounds__(256) void eig_vtu(int64_t n, int p, int tr, int64_t rw, int nblk, int with_w,
                                               const double* __restrict__ V, const double* __restrict__ W,
                                               const double* __restrict__ U, double* __restrict__ part) {
    __shared__ double At[EIG_TILE], Bt[EIG_TILE], red[256];
    const int E = p * p, nall = nblk + with_w;
    const int64_t lo = (int64_t)blockIdx.x * rw, hi = min(n, lo + rw);
    for (int b = 0; b < nall; ++b) {
        const double* src = b < nblk ? V + (int64_t)b * n * p : W;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t t0 = lo; t0 < hi; t0 += tr) {
            const int have = (int)min((int64_t)tr, hi - t0) * p;
            load_tile(At, src + t0 * p, have, tr * p);
            load_tile(Bt, U + t0 * p, have, tr * p);
            __syncthreads();
            tile_products(p, tr, At, Bt, red, acc);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + 256 * i;
            if (e < E) part[((int64_t)blockIdx.x * nall + b) * E + e] = acc[i];
        }
    }
}

// eig_combine<MUL> on W and Q = S_M W in one pass over the rows: outW = W M,
// outQ = Q M (M = R^-1, p x p; S_M (W M) = (S_M W) M needs no product), and
// gpart[block][c][d], the workgroup's share of outW^T outQ. The outputs may be
// the inputs.
__global__ __launch_bounds__(256) void eig_mul2(int64_t n, int p, int tr, int64_t rw, const double* W, const double* Q,
                                                const double* __restrict__ M, double* outW, double* outQ,
                                                double* __restrict__ gpart) {
    __shared__ double At[EIG_TILE], Bt[EIG_TILE], red[256];
    const int E = p * p;
    const int64_t lo = (int64_t)blockIdx.x * rw, hi = min(n, lo + rw);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t0 = lo; t0 < hi; t0 += tr) {
        const int have = (int)min((int64_t)tr, hi - t0) * p;
        load_tile(At, W + t0 * p, have, tr * p);
        load_tile(Bt, Q + t0 * p, have, tr * p);
        __syncthreads();
        double w[8], q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = threadIdx.x + 256 * u;
            w[u] = q[u] = 0.0;
            if (i < have) {
                const int r = i / p, d = i % p;
                for (int c = 0; c < p; ++c) {
                    const double m = M[c * p + d];
                    w[u] = fma(At[r * p + c], m, w[u]);
                    q[u] = fma(Bt[r * p + c], m, q[u]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = threadIdx.x + 256 * u;
            if (i < have) {
                outW[t0 * p + i] = w[u];
                outQ[t0 * p + i] = q[u];
            }
            if (i < tr * p) {
                At[i] = i < have ? w[u] : 0.0;
                Bt[i] = i < have ? q[u] : 0.0;
            }
        }
        __syncthreads();
        tile_products(p, tr, At, Bt, red, acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = threadIdx.x + 256 * i;
        if (e < E) gpart[(int64_t)blockIdx.x * E + e] = acc[i];
    }
}

// eig_resid for r = S y - lambda S_M y: a group takes the row of S, then the
// row of S_M, each in stored order; the partials as eig_resid's
template <typename TA, int G, int KC>
__global__ __launch_bounds__(256) void eig_resid_gen(int64_t n, int64_t k, const int64_t* __restrict__ rp,
                                                     const int32_t* __restrict__ col, const TA* __restrict__ val,
                                                     const int64_t* __restrict__ mrp, const int32_t* __restrict__ mcol,
                                                     const TA* __restrict__ mval, const double* __restrict__ Y,
                                                     const double* __restrict__ lam, double* __restrict__ part) {
    constexpr int GROUPS = 256 / G;
    __shared__ double sh[GROUPS][2 * KC];
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    for (int64_t j0 = 0; j0 < k; j0 += KC) {
        double rr[KC], yy[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) rr[c] = yy[c] = 0.0;
        for (int64_t row0 = (int64_t)blockIdx.x * GROUPS; row0 < n; row0 += (int64_t)gridDim.x * GROUPS) {
            const int64_t row = row0 + grp;
            double acc[KC], accm[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) acc[c] = accm[c] = 0.0;
            if (row < n) {
                const int64_t e1 = rp[row + 1];
                for (int64_t e = rp[row] + lane; e < e1; e += G) {
                    const double v = (double)val[e];
                    const double* yp = Y + (int64_t)col[e] * k + j0;
#pragma unroll
                    for (int c = 0; c < KC; ++c) acc[c] = fma(v, yp[c], acc[c]);
                }
                const int64_t m1 = mrp[row + 1];
                for (int64_t e = mrp[row] + lane; e < m1; e += G) {
                    const double v = (double)mval[e];
                    const double* yp = Y + (int64_t)mcol[e] * k + j0;
#pragma unroll
                    for (int c = 0; c < KC; ++c) accm[c] = fma(v, yp[c], accm[c]);
                }
            }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    acc[c] += __shfl_xor(acc[c], o);
                    accm[c] += __shfl_xor(accm[c], o);
                }
            }
            if (lane == 0 && row < n) {
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const double y = Y[row * k + j0 + c];
                    const double r = fma(-lam[j0 + c], accm[c], acc[c]);
                    rr[c] = fma(r, r, rr[c]);
                    yy[c] = fma(y, y, yy[c]);
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                sh[grp][c] = rr[c];
                sh[grp][KC + c] = yy[c];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * KC) {
            double sum = 0.0;
            for (int g = 0; g < GROUPS; ++g) sum += sh[g][threadIdx.x];
            const int which = threadIdx.x / KC, c = threadIdx.x % KC;
            part[((int64_t)blockIdx.x * 2 + which) * k + j0 + c] = sum;
        }
        __syncthreads();
    }
}

template <typename TA, int G>
int eig_resid_gen_g(unsigned nb, int64_t n, int64_t k, const bsm_sym* S, const bsm_sym* SM, const double* Y,
                    const double* lam, double* part, hipStream_t s) {
    const TA *v = static_cast<const TA*>(S->vals), *mv = static_cast<const TA*>(SM->vals);
    if (k % 4 == 0)
        eig_resid_gen<TA, G, 4><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, SM->rp, SM->col, mv, Y, lam, part);
    else if (k % 2 == 0)
        eig_resid_gen<TA, G, 2><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, SM->rp, SM->col, mv, Y, lam, part);
    else eig_resid_gen<TA, G, 1><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, SM->rp, SM->col, mv, Y, lam, part);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

// G from the longer of the two mean row lengths, the workgroups from n
template <typename TA>
int eig_resid_gen_launch(int64_t n, int64_t k, const bsm_sym* S, const bsm_sym* SM, const double* Y, const double* lam,
                         double* part, unsigned* nb_out, hipStream_t s) {
    const int g = std::max(resid_group(S, n), resid_group(SM, n));
    const unsigned nb = resid_blocks(g, n);
    *nb_out = nb;
    switch (g) {
        case 4: return eig_resid_gen_g<TA, 4>(nb, n, k, S, SM, Y, lam, part, s);
        case 8: return eig_resid_gen_g<TA, 8>(nb, n, k, S, SM, Y, lam, part, s);
        case 16: return eig_resid_gen_g<TA, 16>(nb, n, k, S, SM, Y, lam, part, s);
        default: return eig_resid_gen_g<TA, 64>(nb, n, k, S, SM, Y, lam, part, s);
    }
}

template <typename TA>
int eigsh_gen_t(const bsm_nd_factor* f, const bsm_csr* a, const bsm_sym* S, const bsm_sym* SM, int64_t n, int nev,
                int p, int ncv, double tol, uint64_t seed, const void* v0_dev, void* vec_dev, EigOut& res,
                hipStream_t s) {
    const int E = p * p;
    const size_t np = (size_t)n * (size_t)p;
    const unsigned eb = (unsigned)((np + 255) / 256);
    const EigGeom g = eig_geom(n, p);
    const int maxblk = ncv / p;
    DBuf Vb, Wb, Qb, Tb, Yb, partb, gpartb, Cb, recb, Ub, lamb, sumb;
    DrainOnError drain{s};
    BSM_TRY(Vb.alloc((size_t)ncv * (size_t)n * sizeof(double), s));
    BSM_TRY(Wb.alloc(np * sizeof(double), s));
    BSM_TRY(Qb.alloc(np * sizeof(double), s));  // S_M V_j between the steps, S_M W inside one
    BSM_TRY(Tb.alloc(np * sizeof(double), s));
    BSM_TRY(Yb.alloc(np * sizeof(double), s));
    BSM_TRY(partb.alloc(std::max((size_t)g.nb * (size_t)(maxblk + 1) * E, (size_t)REFINE_MAX_BLOCKS * 2 * p) *
                            sizeof(double), s));
    BSM_TRY(gpartb.alloc((size_t)g.nb * E * sizeof(double), s));
    BSM_TRY(Cb.alloc((size_t)(maxblk + 1) * E * sizeof(double), s));
    BSM_TRY(recb.alloc((size_t)(4 * E + 1 + p) * sizeof(double), s));  // the record, then norm2: one read
    BSM_TRY(Ub.alloc((size_t)E * sizeof(double), s));
    BSM_TRY(lamb.alloc((size_t)p * sizeof(double), s));
    BSM_TRY(sumb.alloc((size_t)2 * p * sizeof(double), s));
    double *V = Vb.as<double>(), *W = Wb.as<double>(), *Q = Qb.as<double>(), *Y = Yb.as<double>();
    double *part = partb.as<double>(), *gpart = gpartb.as<double>(), *C = Cb.as<double>(), *rec = recb.as<double>();
    double *U = Ub.as<double>(), *norm2 = rec + 4 * E + 1, *lamd = lamb.as<double>(), *sums = sumb.as<double>();
    TA* T = Tb.as<TA>();
    std::vector<double> h((size_t)4 * E + 1 + p), B((size_t)E);
    uint32_t flags = 0;

    // C = [V_0 .. V_{nblk-1} (W)]^T Q into C, the record and norm2
    auto project = [&](int nblk, int with_w, int pass) -> int {
        const int nall = nblk + with_w;
        eig_vtu<<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, nblk, with_w, V, W, Q, part);
        BSM_HIP_TRY(hipGetLastError());
        eig_sum<<<1, 256, 0, s>>>((int)g.nb, nall * E, part, C, p, nblk - 1, with_w ? nblk : -1, pass, rec, norm2);
        BSM_HIP_TRY(hipGetLastError());
        return BSM_OK;
    };
    // Cholesky-QR twice on W in the S_M inner product, from the partials of
    // W^T Q in gp; W and Q go through both passes together, into toW and toQ
    auto orthonormalise = [&](const double* gp, double* toW, double* toQ) -> int {
        eig_judge<<<1, 256, 0, s>>>((int)g.nb, p, gp, norm2, 1, rec, U);
        BSM_HIP_TRY(hipGetLastError());
        eig_mul2<<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, W, Q, U, W, Q, gpart);
        BSM_HIP_TRY(hipGetLastError());
        eig_judge<<<1, 256, 0, s>>>((int)g.nb, p, gpart, nullptr, 2, rec, U);
        BSM_HIP_TRY(hipGetLastError());
        eig_mul2<<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, W, Q, U, toW, toQ, gpart);
        BSM_HIP_TRY(hipGetLastError());
        if (read_dev(h.data(), rec, h.size() * sizeof(double), s) != hipSuccess) {
            set_error("eigsh: reading the step's record failed");
            return BSM_ERR_HIP;
        }
        BSM_REQUIRE(eig_mass_pd(p, &h[(size_t)4 * E + 1]), BSM_ERR_UNSUPPORTED,
                    "eigsh: m is not positive definite (w^T S_M w is <= 0 or not finite)");
        return BSM_OK;
    };

    EigLoop loop;
    loop.init(p, nev, ncv, tol);
    if (v0_dev) eig_cast<double, TA><<<eb, 256, 0, s>>>((int64_t)np, static_cast<const TA*>(v0_dev), W);
    else eig_fill<TA><<<eb, 256, 0, s>>>(n, p, seed, W);
    BSM_HIP_TRY(hipGetLastError());
    BSM_TRY(eig_mass_launch<TA>(n, p, SM, W, Q, s));
    stage_mark("eig_mass", s);
    BSM_TRY(project(0, 1, 1));  // W^T Q: the Gram partials, and norm2
    BSM_TRY(orthonormalise(part, V, Q));
    bool have_basis = h[(size_t)4 * E] != 0.0;
    if (!have_basis) flags |= EIG_EXHAUSTED;  // a start block without full rank spans nothing to iterate on
    stage_mark("eig_qr", s);

    const double rtol = refine_default_tol(S->max_len);
    std::vector<uint32_t> it((size_t)p);
    std::vector<double> be((size_t)p);
    while (have_basis) {
        const int j = loop.steps, nblk = j + 1;
        eig_cast<TA, double><<<eb, 256, 0, s>>>((int64_t)np, Q, T);  // Q = S_M V_j
        BSM_HIP_TRY(hipGetLastError());
        BSM_TRY(nd_refine_solve(f, a, (uint64_t)p, T, T, 5, 0.0, it.data(), be.data(), s));
        eig_cast<double, TA><<<eb, 256, 0, s>>>((int64_t)np, T, W);
        BSM_HIP_TRY(hipGetLastError());
        stage_mark("eig_solve", s);  // the stage list is the last solve's, then these (bsm_stage_times)
        for (double e : be)
            if (!(e <= rtol)) flags |= EIG_INEXACT;
        for (int pass = 1; pass <= 2; ++pass) {
            BSM_TRY(eig_mass_launch<TA>(n, p, SM, W, Q, s));
            stage_mark("eig_mass", s);
            BSM_TRY(project(nblk, pass == 1, pass));
            eig_combine<EIG_SUBP><<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, nblk, V, W, C, W, nullptr);
            BSM_HIP_TRY(hipGetLastError());
            stage_mark("eig_reorth", s);
        }
        BSM_TRY(eig_mass_launch<TA>(n, p, SM, W, Q, s));
        stage_mark("eig_mass", s);
        eig_vtu<<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, 0, 1, V, W, Q, part);  // W^T Q after the projections
        BSM_HIP_TRY(hipGetLastError());
        const bool room = (nblk + 1) * p <= ncv;
        BSM_TRY(orthonormalise(part, room ? V + (size_t)nblk * np : W, Q));
        stage_mark("eig_qr", s);
        const bool full = h[(size_t)4 * E] != 0.0;
        if (full) eig_mul_upper(p, &h[(size_t)2 * E], &h[(size_t)E], B.data());
        loop.push(h.data(), full ? B.data() : nullptr);
        if (!full) {
            flags |= EIG_EXHAUSTED;
            loop.ritz(&h[(size_t)3 * E]);
            stage_mark("eig_ritz", s);
            break;
        }
        if (loop.check_due(loop.steps)) {
            loop.ritz();
            stage_mark("eig_ritz", s);  // the stream is idle meanwhile: the host's time
            if (loop.done()) break;
        }
        if (!room) break;
    }
    if (have_basis && loop.m_ritz != loop.m()) loop.ritz();

    // the wanted pairs, lambda ascending
    const int m = loop.m(), got = std::min(nev, m);
    std::vector<int> order((size_t)got);
    std::iota(order.begin(), order.end(), 0);
    std::vector<double> lam_all((size_t)got);
    for (int i = 0; i < got; ++i) lam_all[(size_t)i] = 1.0 / loop.theta_of(i);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lam_all[(size_t)x] < lam_all[(size_t)y]; });
    const double nan = std::numeric_limits<double>::quiet_NaN();
    res.lam.assign((size_t)nev, nan);
    res.resid.assign((size_t)nev, nan);
    if (vec_dev && got < nev) BSM_HIP_TRY(hipMemsetAsync(vec_dev, 0, (size_t)n * (size_t)nev * sizeof(TA), s));
    std::vector<double> Z((size_t)m * p), lamc((size_t)p), sum_h((size_t)2 * p);
    for (int c0 = 0; c0 < got; c0 += p) {
        const int cols = std::min(p, got - c0);
        std::fill(Z.begin(), Z.end(), 0.0);
        std::fill(lamc.begin(), lamc.end(), 0.0);
        for (int c = 0; c < cols; ++c) {
            const int i = order[(size_t)(c0 + c)];
            lamc[(size_t)c] = lam_all[(size_t)i];
            for (int r = 0; r < m; ++r) Z[(size_t)r * p + c] = loop.s_of(i, r);
        }
        BSM_TRY(upload(C, Z.data(), Z.size() * sizeof(double), s));  // C holds (ncv + p) p values
        BSM_TRY(upload(lamd, lamc.data(), lamc.size() * sizeof(double), s));
        eig_combine<EIG_YVZ><<<g.nb, 256, 0, s>>>(n, p, g.tr, g.rw, m / p, V, nullptr, C, Y, nullptr);
        BSM_HIP_TRY(hipGetLastError());
        if constexpr (sizeof(TA) < sizeof(double)) {  // the residual is that of the vectors as they are returned
            eig_cast<TA, double><<<eb, 256, 0, s>>>((int64_t)np, Y, T);
            BSM_HIP_TRY(hipGetLastError());
            eig_cast<double, TA><<<eb, 256, 0, s>>>((int64_t)np, T, Y);
            BSM_HIP_TRY(hipGetLastError());
        }
        unsigned nb = 0;
        BSM_TRY(eig_resid_gen_launch<TA>(n, p, S, SM, Y, lamd, part, &nb, s));
        eig_sum<<<1, 256, 0, s>>>((int)nb, 2 * p, part, sums, p, -1, -1, 0, nullptr, nullptr);
        BSM_HIP_TRY(hipGetLastError());
        BSM_HIP_TRY(read_dev(sum_h.data(), sums, sum_h.size() * sizeof(double), s));
        for (int c = 0; c < cols; ++c) {
            res.lam[(size_t)(c0 + c)] = lamc[(size_t)c];
            res.resid[(size_t)(c0 + c)] = std::sqrt(sum_h[(size_t)c]) / std::sqrt(sum_h[(size_t)(p + c)]);
        }
        if (vec_dev) {
            const unsigned sb = (unsigned)(((size_t)n * cols + 255) / 256);
            eig_store_cols<TA><<<sb, 256, 0, s>>>(n, p, nev, c0, cols, Y, static_cast<TA*>(vec_dev));
            BSM_HIP_TRY(hipGetLastError());
        }
    }
    stage_mark("eig_resid", s);
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    res.info[0] = (uint32_t)loop.steps;
    res.info[1] = (uint32_t)m;
    res.info[2] = have_basis ? (uint32_t)loop.converged() : 0u;
    res.info[3] = flags;
    return BSM_OK;
}

}  // namespace

int nd_eigsh(const bsm_nd_factor* f, const bsm_csr* a, uint64_t nev, uint64_t block, uint64_t ncv, double tol,
             uint64_t seed, const void* v0_dev, double* lam, void* vec_dev, double* resid, uint32_t* info,
             hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(f->mu);
        BSM_REQUIRE(f->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first");
    }
    const int64_t n = (int64_t)f->n;
    EigOut res;
    if (n > 0) {
        // T is dense on the host, ncv x ncv, and the kernels index the basis with int
        BSM_REQUIRE(ncv <= EIG_MAX_NCV, BSM_ERR_UNSUPPORTED, "eigsh: ncv %llu is above %llu",
                    (unsigned long long)ncv, (unsigned long long)EIG_MAX_NCV);
        const bsm_sym* S = nullptr;
        BSM_TRY(sym_obtain(a, s, &S));
        if (tol == 0.0) tol = eig_default_tol(a->dtype == BSM_F64);
        const int rc = a->dtype == BSM_F64 ? eigsh_t<double>(f, a, S, n, (int)nev, (int)block, (int)ncv, tol, seed,
                                                             v0_dev, vec_dev, res, s)
                                           : eigsh_t<float>(f, a, S, n, (int)nev, (int)block, (int)ncv, tol, seed,
                                                            v0_dev, vec_dev, res, s);
        BSM_TRY(rc);
        for (uint64_t i = 0; i < nev; ++i) {  // the outputs are written together, after everything that can fail
            lam[i] = res.lam[i];
            resid[i] = res.resid[i];
        }
    }
    if (info)
        for (int i = 0; i < 4; ++i) info[i] = res.info[i];
    return BSM_OK;
}

int nd_eigsh_gen(const bsm_nd_factor* f, const bsm_csr* a, const bsm_csr* m, uint64_t nev, uint64_t block, uint64_t ncv,
                 double tol, uint64_t seed, const void* v0_dev, double* lam, void* vec_dev, double* resid,
                 uint32_t* info, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(f->mu);
        BSM_REQUIRE(f->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first");
    }
    const int64_t n = (int64_t)f->n;
    EigOut res;
    if (n > 0) {
        BSM_REQUIRE(ncv <= EIG_MAX_NCV, BSM_ERR_UNSUPPORTED, "eigsh: ncv %llu is above %llu",
                    (unsigned long long)ncv, (unsigned long long)EIG_MAX_NCV);
        BSM_REQUIRE(m->nnz > 0, BSM_ERR_UNSUPPORTED, "eigsh: m is not positive definite (it has no stored entries)");
        const bsm_sym *S = nullptr, *SM = nullptr;
        BSM_TRY(sym_obtain(a, s, &S));
        BSM_TRY(sym_obtain(m, s, &SM));
        if (tol == 0.0) tol = eig_default_tol(a->dtype == BSM_F64);
        const int rc = a->dtype == BSM_F64 ? eigsh_gen_t<double>(f, a, S, SM, n, (int)nev, (int)block, (int)ncv, tol,
                                                                 seed, v0_dev, vec_dev, res, s)
                                           : eigsh_gen_t<float>(f, a, S, SM, n, (int)nev, (int)block, (int)ncv, tol,
                                                                seed, v0_dev, vec_dev, res, s);
        BSM_TRY(rc);
        for (uint64_t i = 0; i < nev; ++i) {  // the outputs are written together, after everything that can fail
            lam[i] = res.lam[i];
            resid[i] = res.resid[i];
        }
    }
    if (info)
        for (int i = 0; i < 4; ++i) info[i] = res.info[i];
    return BSM_OK;
}

}  // namespace bsm
