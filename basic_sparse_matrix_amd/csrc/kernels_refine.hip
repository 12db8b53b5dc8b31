// kernels_refine.hip -- mixed-precision use of a kept nd factor (gfx950):
//   convert_values  -- a matrix's values into the factor's dtype (an f32
//                      factor of an f64 matrix, bsm_nd_factor_create_as)
//   sym_obtain      -- S, the symmetric matrix the factor stands for: a's
//                      stored entries with column <= row, mirrored; built once
//                      per handle and cached on it
//   nd_refine_solve -- iterative refinement (bsm_nd_factor_solve_refined):
//                      x = M^-1 b by the factor, then corrections from f64
//                      residuals R = B - S X until the backward error
//                      omega_j = ||r_j||inf / (||S||inf ||x_j||inf + ||b_j||inf)
//                      of every column is below tol or stops halving
// Every column is on its own: the sums of a (row, column) never depend on k,
// the maxima are taken on bit patterns (order-free, and a NaN is the largest),
// there are no floating-point atomics: the same call gives the same bits.
#include <algorithm>
#include <vector>

#include "bsm_internal.hpp"
#include "refine_rule.hpp"

namespace bsm {
namespace {

inline unsigned blocks_for(uint64_t n, unsigned b, uint64_t cap = 0x7fffffffu) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + b - 1) / b, cap));
}

// ---- values into another float dtype ---------------------------------------
// four values per thread: 2 x 16 bytes of f64 against 16 bytes of f32,
// round-to-nearest-even; the last n % 4 one by one
__global__ __launch_bounds__(256) void convert_f64_f32(uint64_t n, const double* __restrict__ src,
                                                       float* __restrict__ dst) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x, i = q * 4;
    if (i + 4 <= n) {
        const double2 a = reinterpret_cast<const double2*>(src)[q * 2];
        const double2 b = reinterpret_cast<const double2*>(src)[q * 2 + 1];
        reinterpret_cast<float4*>(dst)[q] = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
    } else {
        for (uint64_t t = i; t < n; ++t) dst[t] = (float)src[t];
    }
}
__global__ __launch_bounds__(256) void convert_f32_f64(uint64_t n, const float* __restrict__ src,
                                                       double* __restrict__ dst) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x, i = q * 4;
    if (i + 4 <= n) {
        const float4 a = reinterpret_cast<const float4*>(src)[q];
        reinterpret_cast<double2*>(dst)[q * 2] = make_double2((double)a.x, (double)a.y);
        reinterpret_cast<double2*>(dst)[q * 2 + 1] = make_double2((double)a.z, (double)a.w);
    } else {
        for (uint64_t t = i; t < n; ++t) dst[t] = (double)src[t];
    }
}

// ---- the symmetric copy ----------------------------------------------------
// per row: the entries with column < row (they are transposed) and <= row
__global__ __launch_bounds__(256) void sym_count(int64_t n, const int64_t* __restrict__ rp,
                                                 const int32_t* __restrict__ col, int32_t* __restrict__ strict,
                                                 int32_t* __restrict__ le) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t a = 0, b = 0;
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
        a += col[e] < i;
        b += col[e] <= i;
    }
    strict[i] = a;
    le[i] = b;
}

template <typename T>
__global__ __launch_bounds__(256) void sym_fill_lower(int64_t n, const int64_t* __restrict__ rp,
                                                      const int32_t* __restrict__ col, const T* __restrict__ val,
                                                      const int64_t* __restrict__ lrp, int32_t* __restrict__ lcol,
                                                      T* __restrict__ lval) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t at = lrp[i];
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e)
        if (col[e] < i) {
            lcol[at] = col[e];
            lval[at] = val[e];
            ++at;
        }
}

__global__ __launch_bounds__(256) void sym_len(int64_t n, const int32_t* __restrict__ le,
                                               const int64_t* __restrict__ urp, int32_t* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) len[i] = le[i] + (int32_t)(urp[i + 1] - urp[i]);
}

// row i of S: a's entries with column <= i in stored order, then row i of the
// transposed strict lower triangle (columns > i, ascending). stats[0]: the
// largest row sum of |values| (as bits), stats[1]: the longest row -- integer
// maxima, whose result no order changes.
template <typename T>
__global__ __launch_bounds__(256) void sym_fill(int64_t n, const int64_t* __restrict__ rp,
                                                const int32_t* __restrict__ col, const T* __restrict__ val,
                                                const int64_t* __restrict__ urp, const int32_t* __restrict__ ucol,
                                                const T* __restrict__ uval, const int64_t* __restrict__ srp,
                                                int32_t* __restrict__ scol, T* __restrict__ sval,
                                                ull* __restrict__ stats) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t at = srp[i];
    double sum = 0.0;
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e)
        if (col[e] <= i) {
            scol[at] = col[e];
            sval[at] = val[e];
            sum += fabs((double)val[e]);
            ++at;
        }
    for (int64_t e = urp[i]; e < urp[i + 1]; ++e) {
        scol[at] = ucol[e];
        sval[at] = uval[e];
        sum += fabs((double)uval[e]);
        ++at;
    }
    atomicMax(stats, abs_bits(sum));
    atomicMax(stats + 1, (ull)(at - srp[i]));
}

void sym_free(bsm_sym* m) {
    if (!m) return;
    if (m->rp) (void)hipFree(m->rp);
    if (m->col) (void)hipFree(m->col);
    if (m->vals) (void)hipFree(m->vals);
    delete m;
}

int sym_build(const bsm_csr* a, hipStream_t s, bsm_sym** out) {
    const int64_t n = (int64_t)a->rows;
    const size_t es = dtype_size(a->dtype);
    const unsigned rb = blocks_for((uint64_t)n, 256);
    DBuf strict, le, len, rp_tmp, ws, stats;
    DrainOnError drain{s};
    BSM_TRY(strict.alloc((size_t)n * sizeof(int32_t), s));
    BSM_TRY(le.alloc((size_t)n * sizeof(int32_t), s));
    BSM_TRY(len.alloc((size_t)n * sizeof(int32_t), s));
    BSM_TRY(rp_tmp.alloc(((size_t)n + 1) * sizeof(int64_t), s));
    BSM_TRY(ws.alloc(scan_workspace_bytes((uint64_t)n), s));
    BSM_TRY(stats.alloc(2 * sizeof(ull), s));
    sym_count<<<rb, 256, 0, s>>>(n, a->row_ptr, a->col, strict.as<int32_t>(), le.as<int32_t>());
    BSM_HIP_TRY(hipGetLastError());
    BSM_TRY(exclusive_scan_i32_to_i64(strict.as<int32_t>(), rp_tmp.as<int64_t>(), (uint64_t)n, ws.p, ws.bytes, s));
    int64_t nnz_l = 0;
    BSM_HIP_TRY(read_dev(&nnz_l, rp_tmp.as<int64_t>() + n, sizeof(int64_t), s));
    // the strict lower triangle as a Csr of its own, and its transpose
    bsm_csr *low = nullptr, *up = nullptr;
    struct Guard {
        bsm_csr *&low, *&up;
        ~Guard() {
            bsm_csr_free(low);
            bsm_csr_free(up);
        }
    } guard{low, up};
    BSM_TRY(csr_alloc(&low, a->dtype, (uint64_t)n, (uint64_t)n, (uint64_t)nnz_l));
    BSM_HIP_TRY(hipMemcpyAsync(low->row_ptr, rp_tmp.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    const int rc_fill = dispatch_dtype(a->dtype, [&]<typename T>() -> int {
        if constexpr (IsFloat<T>::value) {
            sym_fill_lower<T><<<rb, 256, 0, s>>>(n, a->row_ptr, a->col, static_cast<const T*>(a->vals), low->row_ptr,
                                                 low->col, static_cast<T*>(low->vals));
            BSM_HIP_TRY(hipGetLastError());
            return BSM_OK;
        } else {
            set_error("refined solve: f32/f64 only");
            return BSM_ERR_INVALID;
        }
    });
    BSM_TRY(rc_fill);
    BSM_TRY(transpose_dispatch(low, &up, s));
    // S's row lengths, row_ptr, then the rows
    sym_len<<<rb, 256, 0, s>>>(n, le.as<int32_t>(), up->row_ptr, len.as<int32_t>());
    BSM_HIP_TRY(hipGetLastError());
    BSM_TRY(exclusive_scan_i32_to_i64(len.as<int32_t>(), rp_tmp.as<int64_t>(), (uint64_t)n, ws.p, ws.bytes, s));
    int64_t nnz_s = 0;
    BSM_HIP_TRY(read_dev(&nnz_s, rp_tmp.as<int64_t>() + n, sizeof(int64_t), s));
    std::unique_ptr<bsm_sym, void (*)(bsm_sym*)> m(new bsm_sym, sym_free);
    m->nnz = (uint64_t)nnz_s;
    DBuf o_rp, o_col, o_val;  // plain allocations: they live as long as the handle
    BSM_TRY(o_rp.alloc(((size_t)n + 1) * sizeof(int64_t)));
    m->rp = static_cast<int64_t*>(o_rp.release());
    BSM_TRY(o_col.alloc((size_t)nnz_s * sizeof(int32_t)));
    m->col = static_cast<int32_t*>(o_col.release());
    BSM_TRY(o_val.alloc((size_t)nnz_s * es));
    m->vals = o_val.release();
    BSM_HIP_TRY(hipMemcpyAsync(m->rp, rp_tmp.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    BSM_HIP_TRY(hipMemsetAsync(stats.p, 0, 2 * sizeof(ull), s));
    const int rc_sym = dispatch_dtype(a->dtype, [&]<typename T>() -> int {
        if constexpr (IsFloat<T>::value) {
            sym_fill<T><<<rb, 256, 0, s>>>(n, a->row_ptr, a->col, static_cast<const T*>(a->vals), up->row_ptr, up->col,
                                           static_cast<const T*>(up->vals), m->rp, m->col, static_cast<T*>(m->vals),
                                           stats.as<ull>());
            BSM_HIP_TRY(hipGetLastError());
        }
        return BSM_OK;
    });
    BSM_TRY(rc_sym);
    ull h[2] = {0, 0};
    BSM_HIP_TRY(read_dev(h, stats.p, sizeof(h), s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    std::memcpy(&m->norm_inf, &h[0], sizeof(double));
    m->max_len = h[1];
    *out = m.release();
    return BSM_OK;
}

// ---- the refinement's kernels ----------------------------------------------
// B = (double)b, and per workgroup and column max |b|: part[block][j]
template <typename TA>
__global__ __launch_bounds__(256) void refine_load(int64_t n, int64_t k, const TA* __restrict__ b,
                                                   double* __restrict__ B, ull* __restrict__ part) {
    __shared__ ull sh[256];
    for (int64_t j = 0; j < k; ++j) {
        ull m = 0;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
            const double v = (double)b[i * k + j];
            B[i * k + j] = v;
            m = umax(m, abs_bits(v));
        }
        sh[threadIdx.x] = m;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] = umax(sh[threadIdx.x], sh[threadIdx.x + o]);
            __syncthreads();
        }
        if (threadIdx.x == 0) part[(int64_t)blockIdx.x * k + j] = sh[0];
        __syncthreads();
    }
}

// the largest of part[b * stride + idx], b < nb, in thread 0 (one workgroup of 256)
__device__ __forceinline__ ull reduce_partials(const ull* __restrict__ part, int nb, int64_t stride, int64_t idx,
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

// ||b_j||inf and the first solve's scale; every column but a zero one is solved
__global__ __launch_bounds__(256) void refine_begin(int nb, int64_t k, const ull* __restrict__ part,
                                                    RefineCol* __restrict__ st) {
    __shared__ ull sh[256];
    for (int64_t j = 0; j < k; ++j) {
        const ull m = reduce_partials(part, nb, k, j, sh);
        if (threadIdx.x == 0) {
            RefineCol c;
            c.bnorm = bits_abs(m);
            c.scale = refine_scale(c.bnorm);
            c.zero = c.bnorm == 0.0;
            c.active = !c.zero;
            st[j] = c;
        }
    }
}

// W = V / scale in the factor's dtype on the active columns, 0 on the others
template <typename TF>
__global__ __launch_bounds__(256) void refine_scale_cast(int64_t n, int64_t k, const double* __restrict__ V,
                                                         const RefineCol* __restrict__ st, TF* __restrict__ W) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k) return;
    const RefineCol& c = st[i % k];
    W[i] = c.active ? (TF)(V[i] / c.scale) : (TF)0;
}

// first: X = scale D. Later, on the active columns: the iterate kept in Xp,
// X = X + scale D (scale is a power of two: the product is exact)
template <typename TF>
__global__ __launch_bounds__(256) void refine_update(int64_t n, int64_t k, const TF* __restrict__ D,
                                                     const RefineCol* __restrict__ st, double* __restrict__ X,
                                                     double* __restrict__ Xp, bool first) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k) return;
    const RefineCol& c = st[i % k];
    if (first) {
        X[i] = c.zero ? 0.0 : c.scale * (double)D[i];
    } else if (c.active) {
        const double x = X[i];
        Xp[i] = x;
        X[i] = x + c.scale * (double)D[i];
    }
}

// R = B - S X, X / B / R f64 row-major n x k. G lanes per row; a lane takes
// the row's entries lane, lane + G, ... in stored order and, for each, the KC
// contiguous values of X's row (16-byte loads for KC = 2 and 4); the group's
// sums meet in a fixed xor tree. part[block][0][j] = max |r_j|,
// part[block][1][j] = max |x_j| over the workgroup's rows.
template <typename TA, int G, int KC>
__global__ __launch_bounds__(256) void refine_resid(int64_t n, int64_t k, const int64_t* __restrict__ rp,
                                                    const int32_t* __restrict__ col, const TA* __restrict__ val,
                                                    const double* __restrict__ X, const double* __restrict__ B,
                                                    double* __restrict__ R, ull* __restrict__ part) {
    constexpr int GROUPS = 256 / G;
    __shared__ ull sh[GROUPS][2 * KC];
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    for (int64_t j0 = 0; j0 < k; j0 += KC) {
        ull mr[KC], mx[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) mr[c] = mx[c] = 0;
        for (int64_t row0 = (int64_t)blockIdx.x * GROUPS; row0 < n; row0 += (int64_t)gridDim.x * GROUPS) {
            const int64_t row = row0 + grp;
            double acc[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) acc[c] = 0.0;
            if (row < n) {
                const int64_t e1 = rp[row + 1];
                for (int64_t e = rp[row] + lane; e < e1; e += G) {
                    const double v = (double)val[e];
                    const double* xp = X + (int64_t)col[e] * k + j0;
                    double xv[KC];
                    if constexpr (KC == 1) {
                        xv[0] = xp[0];
                    } else {
#pragma unroll
                        for (int c = 0; c < KC; c += 2) {
                            const double2 t = *reinterpret_cast<const double2*>(xp + c);
                            xv[c] = t.x;
                            xv[c + 1] = t.y;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < KC; ++c) acc[c] = fma(v, xv[c], acc[c]);
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
                    const int64_t at = row * k + j0 + c;
                    const double r = B[at] - acc[c];
                    R[at] = r;
                    mr[c] = umax(mr[c], abs_bits(r));
                    mx[c] = umax(mx[c], abs_bits(X[at]));
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                sh[grp][c] = mr[c];
                sh[grp][KC + c] = mx[c];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * KC) {
            ull m = 0;
            for (int g = 0; g < GROUPS; ++g) m = umax(m, sh[g][threadIdx.x]);
            const int which = threadIdx.x / KC, c = threadIdx.x % KC;
            part[((int64_t)blockIdx.x * 2 + which) * k + j0 + c] = m;
        }
        __syncthreads();
    }
}

// the partials into omega_j, then the column's rule (refine_rule.hpp): the
// first iterate for it == 0, correction `it` afterwards
__global__ __launch_bounds__(256) void refine_judge(int nb, int64_t k, const ull* __restrict__ part, double snorm,
                                                    double tol, uint32_t it, RefineCol* __restrict__ st) {
    __shared__ ull sh[256];
    for (int64_t j = 0; j < k; ++j) {
        const ull br = reduce_partials(part, nb, 2 * k, j, sh);
        const ull bx = reduce_partials(part, nb, 2 * k, k + j, sh);
        if (threadIdx.x == 0) {
            RefineCol c = st[j];
            const double rmax = bits_abs(br), xmax = bits_abs(bx);
            const double omega = refine_omega(rmax, xmax, c.bnorm, snorm);
            if (it == 0) refine_rule_init(c, c.bnorm, omega, rmax, tol);
            else refine_rule_step(c, it, omega, rmax, tol);
            st[j] = c;
        }
    }
}

// x = the best iterate in a's dtype
template <typename TA>
__global__ __launch_bounds__(256) void refine_finish(int64_t n, int64_t k, const double* __restrict__ X,
                                                     const double* __restrict__ Xp, const RefineCol* __restrict__ st,
                                                     TA* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k) return;
    const RefineCol& c = st[i % k];
    x[i] = c.zero ? (TA)0 : (TA)(c.use_prev ? Xp[i] : X[i]);
}

template <typename TA, int G>
int resid_launch_g(unsigned nb, int64_t n, int64_t k, const bsm_sym* S, const double* X, const double* B, double* R,
                   ull* part, hipStream_t s) {
    const TA* v = static_cast<const TA*>(S->vals);
    if (k % 4 == 0) refine_resid<TA, G, 4><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, X, B, R, part);
    else if (k % 2 == 0) refine_resid<TA, G, 2><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, X, B, R, part);
    else refine_resid<TA, G, 1><<<nb, 256, 0, s>>>(n, k, S->rp, S->col, v, X, B, R, part);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

template <typename TA>
int resid_launch(int64_t n, int64_t k, const bsm_sym* S, const double* X, const double* B, double* R, ull* part,
                 unsigned* nb_out, hipStream_t s) {
    const int g = resid_group(S, n);
    const unsigned nb = resid_blocks(g, n);
    *nb_out = nb;
    switch (g) {
        case 4: return resid_launch_g<TA, 4>(nb, n, k, S, X, B, R, part, s);
        case 8: return resid_launch_g<TA, 8>(nb, n, k, S, X, B, R, part, s);
        case 16: return resid_launch_g<TA, 16>(nb, n, k, S, X, B, R, part, s);
        default: return resid_launch_g<TA, 64>(nb, n, k, S, X, B, R, part, s);
    }
}

template <typename TA, typename TF>
int refine_t(const bsm_nd_factor* f, const bsm_sym* S, int64_t n, int64_t k, const void* b_dev, void* x_dev,
             uint32_t max_iter, double tol, std::vector<RefineCol>& cols, hipStream_t s) {
    const size_t nk = (size_t)n * (size_t)k;
    const unsigned eb = blocks_for(nk, 256);
    const unsigned lb = blocks_for((uint64_t)n, 256, REFINE_MAX_BLOCKS);
    DBuf Bb, Xb, Xpb, Rb, Wb, partb, stb;
    DrainOnError drain{s};
    BSM_TRY(Bb.alloc(nk * sizeof(double), s));
    BSM_TRY(Xb.alloc(nk * sizeof(double), s));
    BSM_TRY(Xpb.alloc(nk * sizeof(double), s));
    BSM_TRY(Rb.alloc(nk * sizeof(double), s));
    BSM_TRY(Wb.alloc(nk * sizeof(TF), s));
    BSM_TRY(partb.alloc((size_t)REFINE_MAX_BLOCKS * 2 * (size_t)k * sizeof(ull), s));
    BSM_TRY(stb.alloc((size_t)k * sizeof(RefineCol), s));
    double *B = Bb.as<double>(), *X = Xb.as<double>(), *Xp = Xpb.as<double>(), *R = Rb.as<double>();
    TF* W = Wb.as<TF>();
    ull* part = partb.as<ull>();
    RefineCol* st = stb.as<RefineCol>();

    refine_load<TA><<<lb, 256, 0, s>>>(n, k, static_cast<const TA*>(b_dev), B, part);
    BSM_HIP_TRY(hipGetLastError());
    refine_begin<<<1, 256, 0, s>>>((int)lb, k, part, st);
    BSM_HIP_TRY(hipGetLastError());
    for (uint32_t it = 0;; ++it) {
        refine_scale_cast<TF><<<eb, 256, 0, s>>>(n, k, it == 0 ? B : R, st, W);
        BSM_HIP_TRY(hipGetLastError());
        BSM_TRY(nd_factor_solve(f, BSM_ND_SYS_A, (uint64_t)k, (uint64_t)n, W, W, s));  // all k columns, in place
        refine_update<TF><<<eb, 256, 0, s>>>(n, k, W, st, X, Xp, it == 0);
        BSM_HIP_TRY(hipGetLastError());
        stage_mark("refine_update", s);  // the stage list is the last solve's, then these (bsm_stage_times)
        unsigned nb = 0;
        BSM_TRY(resid_launch<TA>(n, k, S, X, B, R, part, &nb, s));
        stage_mark("refine_resid", s);
        refine_judge<<<1, 256, 0, s>>>((int)nb, k, part, S->norm_inf, tol, it, st);
        BSM_HIP_TRY(hipGetLastError());
        stage_mark("refine_judge", s);
        BSM_HIP_TRY(read_dev(cols.data(), st, (size_t)k * sizeof(RefineCol), s));
        bool any = false;
        for (const RefineCol& c : cols) any = any || c.active;
        if (!any || it >= max_iter) break;
    }
    refine_finish<TA><<<eb, 256, 0, s>>>(n, k, X, Xp, st, static_cast<TA*>(x_dev));
    BSM_HIP_TRY(hipGetLastError());
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    return BSM_OK;
}

}  // namespace

void sym_destroy(bsm_sym* m) { sym_free(m); }

// the handle's symmetric copy, built on first use
int sym_obtain(const bsm_csr* a, hipStream_t s, const bsm_sym** out) {
    std::lock_guard<std::mutex> lk(a->plan_mu);
    if (!a->sym) {
        bsm_sym* m = nullptr;
        BSM_TRY(sym_build(a, s, &m));
        a->sym = m;
    }
    *out = a->sym;
    return BSM_OK;
}

// lanes per row from S's mean row length (a property of the matrix alone, so
// a column's sums do not move with k)
int resid_group(const bsm_sym* S, int64_t n) {
    const uint64_t mean = S->nnz / (uint64_t)std::max<int64_t>(n, 1);
    return mean <= 4 ? 4 : mean <= 8 ? 8 : mean <= 16 ? 16 : 64;
}
unsigned resid_blocks(int g, int64_t n) { return blocks_for((uint64_t)n, 256u / (unsigned)g, REFINE_MAX_BLOCKS); }

// ---- what the pcg solve takes from here (bsm_internal.hpp) -------------------
namespace {
template <typename TA, typename TF>
int first_iterate_t(const bsm_nd_factor* f, const bsm_sym* S, int64_t n, int64_t k, const void* b_dev, double* B,
                    double* X, double* R, TF* W, ull* part, RefineCol* st, unsigned* nb, hipStream_t s) {
    const unsigned eb = blocks_for((uint64_t)n * (uint64_t)k, 256);
    const unsigned lb = blocks_for((uint64_t)n, 256, REFINE_MAX_BLOCKS);
    refine_load<TA><<<lb, 256, 0, s>>>(n, k, static_cast<const TA*>(b_dev), B, part);
    BSM_HIP_TRY(hipGetLastError());
    refine_begin<<<1, 256, 0, s>>>((int)lb, k, part, st);
    BSM_HIP_TRY(hipGetLastError());
    refine_scale_cast<TF><<<eb, 256, 0, s>>>(n, k, B, st, W);
    BSM_HIP_TRY(hipGetLastError());
    BSM_TRY(nd_factor_solve(f, BSM_ND_SYS_A, (uint64_t)k, (uint64_t)n, W, W, s));
    refine_update<TF><<<eb, 256, 0, s>>>(n, k, W, st, X, nullptr, true);
    BSM_HIP_TRY(hipGetLastError());
    return resid_launch<TA>(n, k, S, X, B, R, part, nb, s);
}
}  // namespace

int refine_first_iterate(const bsm_nd_factor* f, const bsm_csr* a, const bsm_sym* S, int64_t n, int64_t k,
                         const void* b_dev, double* B, double* X, double* R, void* W, ull* part, RefineCol* st,
                         unsigned* nb, hipStream_t s) {
    if (a->dtype == BSM_F64)
        return f->dtype == BSM_F64
                   ? first_iterate_t<double, double>(f, S, n, k, b_dev, B, X, R, static_cast<double*>(W), part, st, nb, s)
                   : first_iterate_t<double, float>(f, S, n, k, b_dev, B, X, R, static_cast<float*>(W), part, st, nb, s);
    return f->dtype == BSM_F64
               ? first_iterate_t<float, double>(f, S, n, k, b_dev, B, X, R, static_cast<double*>(W), part, st, nb, s)
               : first_iterate_t<float, float>(f, S, n, k, b_dev, B, X, R, static_cast<float*>(W), part, st, nb, s);
}

int refine_precondition(const bsm_nd_factor* f, int64_t n, int64_t k, const double* V, const RefineCol* st, void* W,
                        hipStream_t s) {
    const unsigned eb = blocks_for((uint64_t)n * (uint64_t)k, 256);
    if (f->dtype == BSM_F64) refine_scale_cast<double><<<eb, 256, 0, s>>>(n, k, V, st, static_cast<double*>(W));
    else refine_scale_cast<float><<<eb, 256, 0, s>>>(n, k, V, st, static_cast<float*>(W));
    BSM_HIP_TRY(hipGetLastError());
    return nd_factor_solve(f, BSM_ND_SYS_A, (uint64_t)k, (uint64_t)n, W, W, s);
}

int refine_residual(const bsm_csr* a, const bsm_sym* S, int64_t n, int64_t k, const double* X, const double* B,
                    double* R, ull* part, unsigned* nb, hipStream_t s) {
    return a->dtype == BSM_F64 ? resid_launch<double>(n, k, S, X, B, R, part, nb, s)
                               : resid_launch<float>(n, k, S, X, B, R, part, nb, s);
}

int convert_values(int src_dtype, int dst_dtype, uint64_t n, const void* src, void* dst, hipStream_t s) {
    if (n == 0) return BSM_OK;
    const unsigned nb = blocks_for((n + 3) / 4, 256);
    if (src_dtype == BSM_F64 && dst_dtype == BSM_F32)
        convert_f64_f32<<<nb, 256, 0, s>>>(n, static_cast<const double*>(src), static_cast<float*>(dst));
    else if (src_dtype == BSM_F32 && dst_dtype == BSM_F64)
        convert_f32_f64<<<nb, 256, 0, s>>>(n, static_cast<const float*>(src), static_cast<double*>(dst));
    else {
        set_error("convert_values: dtype %d to %d", src_dtype, dst_dtype);
        return BSM_ERR_INVALID;
    }
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

int nd_refine_solve(const bsm_nd_factor* f, const bsm_csr* a, uint64_t k, const void* b_dev, void* x_dev,
                    uint32_t max_iter, double tol, uint32_t* iters, double* berr, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(f->mu);
        BSM_REQUIRE(f->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first");
    }
    const int64_t n = (int64_t)f->n;
    std::vector<RefineCol> cols((size_t)k);
    if (n > 0 && k > 0) {
        BSM_REQUIRE(k < ((uint64_t)1 << 31), BSM_ERR_UNSUPPORTED, "refined solve: k >= 2^31");
        const bsm_sym* S = nullptr;
        BSM_TRY(sym_obtain(a, s, &S));
        if (tol == 0.0) tol = refine_default_tol(S->max_len);
        int rc;
        if (a->dtype == BSM_F64)
            rc = f->dtype == BSM_F64
                     ? refine_t<double, double>(f, S, n, (int64_t)k, b_dev, x_dev, max_iter, tol, cols, s)
                     : refine_t<double, float>(f, S, n, (int64_t)k, b_dev, x_dev, max_iter, tol, cols, s);
        else
            rc = f->dtype == BSM_F64
                     ? refine_t<float, double>(f, S, n, (int64_t)k, b_dev, x_dev, max_iter, tol, cols, s)
                     : refine_t<float, float>(f, S, n, (int64_t)k, b_dev, x_dev, max_iter, tol, cols, s);
        BSM_TRY(rc);
    }
    for (uint64_t j = 0; j < k; ++j) {
        if (iters) iters[j] = cols[j].iters;
        if (berr) berr[j] = cols[j].best;
    }
    return BSM_OK;
}

}  // namespace bsm
