/*
 * bsm.h -- C-ABI of the MI355X-native sparse-matrix hot path
 * (libbsm_hip.so, built from basic_sparse_matrix_amd/csrc/).
 *
 * This is the drop-in boundary for the reference crate
 * jamieapps101/Basic_Sparse_Matrix (pure Rust). The reference has no FFI of
 * its own; these are the entry points its hot-path methods would bind
 * through `extern "C"` (see INTEGRATION.md for the Rust-side binding). Every
 * function below names the reference item it replaces.
 *
 * Conventions
 *  - Plain pointers and sizes only; indices are uint64_t like Rust's usize.
 *  - Host-buffer entry points (bsm_csr_*, bsm_solve, ...) are synchronous:
 *    when they return, device work is complete and output host buffers are
 *    filled. The library NEVER takes ownership of caller memory; device
 *    memory is owned by opaque handles released with bsm_csr_free.
 *  - Device entry points (bsm_dev_*) take device (HBM) pointers and a
 *    hipStream_t passed as void*; they enqueue work and return immediately.
 *  - Return value: BSM_OK (0) or a bsm_status; bsm_last_error() gives a
 *    thread-local message. Dimension checks that the reference answers with
 *    Err(MatErr::...) are repeated here (BSM_ERR_DIMENSIONS /
 *    BSM_ERR_NON_SQUARE) but callers are expected to check first, as the
 *    reference does, so that Err values stay identical.
 *  - Arithmetic: floating point is IEEE with no FMA contraction and the
 *    reference's summation order (bit-exact); integers wrap
 *    (reference bench profile overflow-checks=false, Cargo.toml:18).
 *  - Device CSR layout: row_ptr int64[rows+1], col int32[nnz] (so cols must
 *    be < 2^31), values T[nnz]. Dense operands on device are ROW-major
 *    (n x k, element (r,j) at r*k + j) so one CSR entry gathers k contiguous
 *    values; host Dense operands are the reference's column list
 *    (Vec<Vec<T>>, dense.rs:8) passed as an array of k column pointers.
 */
#ifndef BSM_H
#define BSM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSM_API_VERSION 1

/* Scalar types of the reference's generic T that run on the GPU. */
typedef enum bsm_dtype {
    BSM_F64 = 0,
    BSM_F32 = 1,
    BSM_I32 = 2,
    BSM_U32 = 3,
    BSM_I64 = 4,
    BSM_U64 = 5
} bsm_dtype;

typedef enum bsm_status {
    BSM_OK = 0,
    BSM_ERR_INVALID = 1,     /* bad argument (null pointer, unknown dtype, ...) */
    BSM_ERR_DIMENSIONS = 2,  /* MatErr::IncorrectDimensions (util.rs:51) */
    BSM_ERR_NON_SQUARE = 3,  /* MatErr::NonSquareMatrix (util.rs:50) */
    BSM_ERR_PANIC = 4,       /* input on which the reference panics (OOB index, empty row) */
    BSM_ERR_HIP = 5,         /* HIP runtime error */
    BSM_ERR_OOM = 6,         /* device allocation failed */
    BSM_ERR_UNSUPPORTED = 7, /* valid input outside what this build implements */
    BSM_ERR_NO_DEVICE = 8,   /* no usable gfx950 device */
    BSM_ERR_OUT_OF_BOUNDS = 9, /* MatErr::OutOfBounds (util.rs:54; COO::insert, sparse.rs:45-53) */
    BSM_ERR_COMM = 10          /* RCCL error (multi-GPU entry points) */
} bsm_status;

/* Opaque device-resident CSR matrix (a finalised Csr<T>, sparse.rs:68-78). */
typedef struct bsm_csr bsm_csr;

/* ---- library ------------------------------------------------------------ */
int bsm_api_version(void);
/* Thread-local description of the last failure on this thread. */
const char* bsm_last_error(void);
/* Device time of the stages of the last bsm_solve / bsm_solve_blocked /
 * bsm_csr_cholesky on this thread (HIP events on its stream): *n stages; the
 * first min(max, *n) names (32 chars each, NUL-terminated) and durations in
 * ms. Diagnostic, recorded only while armed by bsm_stage_timing(1) (or env
 * BSM_STAGE_TIMES=1). */
int bsm_stage_timing(int on);
int bsm_stage_times(int max, int* n, char* names, double* ms);
int bsm_device_count(int* n);
/* Select the device used by subsequent calls on this thread. */
int bsm_set_device(int ordinal);

/* ---- device-resident CSR handles ---------------------------------------- */
/* Upload a finalised Csr<T> (sparse.rs:68-78: row_index = row_ptr of length
 * rows+1, col_index, v). Replaces nothing in the reference: it is the
 * marshalling step a Rust `mul_dense` performs before the kernel call (the
 * handle can be cached by the caller because a finalised Csr is immutable:
 * insert returns Err(MatrixFinalised), sparse.rs:223-225). */
int bsm_csr_upload(int dtype, uint64_t rows, uint64_t cols, uint64_t nnz,
                   const uint64_t* row_ptr, const uint64_t* col_idx, const void* vals,
                   bsm_csr** out);
/* Build a finalised Csr on the device from a SEQUENCE of Csr::insert(v[i],
 * row[i], col[i]) calls followed by finalise (sparse.rs:206-250): zero
 * values are skipped, an entry belongs to the running maximum of the rows
 * inserted so far (insert_unchecked, sparse.rs:237-250), skipped rows get
 * empty ranges, and finalise pads row_index. A kept row >= rows is the
 * reference's finalise panic ("big eek", sparse.rs:210) -> BSM_ERR_PANIC;
 * a kept col >= cols -> BSM_ERR_PANIC (the device Csr holds in-bounds
 * columns). Host arrays of n entries. */
int bsm_csr_from_inserts(int dtype, uint64_t rows, uint64_t cols, uint64_t n, const uint64_t* row,
                         const uint64_t* col, const void* vals, bsm_csr** out);
/* From<COO<T>> for Csr<T> (sparse.rs:56-66): the n COO entries (row[i],
 * col[i], vals[i]) in insert order, stably sorted by (row, col) (Rust's
 * sort_by is stable), then inserted (zero skip) and finalised. The
 * reference's per-entry println! is not reproduced. An entry outside dims
 * (COO::insert would have returned Err(OutOfBounds)) -> BSM_ERR_OUT_OF_BOUNDS.
 * Host arrays. */
int bsm_csr_from_coo(int dtype, uint64_t rows, uint64_t cols, uint64_t n, const uint64_t* row,
                     const uint64_t* col, const void* vals, bsm_csr** out);
int bsm_csr_shape(const bsm_csr* m, uint64_t* rows, uint64_t* cols, uint64_t* nnz,
                  int* dtype);
/* Copy a handle back into caller-allocated host arrays (rows+1, nnz, nnz).
 * A small bsm_csr_mul_dense result (at most 8,192 rows and 131,072 row x
 * column slots) carries a host copy written by the same kernel as its device
 * arrays: its download is a host copy with no device work. */
int bsm_csr_download(const bsm_csr* m, uint64_t* row_ptr, uint64_t* col_idx, void* vals);
/* Page-lock (hipHostRegister) / release a caller-owned host range that result
 * arrays are downloaded into again and again (this build's addition; no
 * reference counterpart). bsm_csr_download into registered arrays is one
 * direct DMA per array, the columns widened to usize on the device; into
 * pageable arrays it stages through pinned buffers. The Python mirror's host
 * result pool (hostpool.py) registers its mappings once. */
int bsm_host_register(void* p, uint64_t bytes);
int bsm_host_unregister(void* p);
void bsm_csr_free(bsm_csr* m);

/* ---- hot path (host buffers in/out, synchronous) ------------------------- */
/* Csr::mul_dense (sparse.rs:426-446) and Csr::mul_dense_s (sparse.rs:448-466):
 * out = a * X as a new finalised Csr with dims (rows, k), zero results
 * dropped (sparse.rs:229). X is k columns of x_rows values each
 * (Dense::get_col, dense.rs:31-33). x_rows != cols -> BSM_ERR_DIMENSIONS. */
int bsm_csr_mul_dense(const bsm_csr* a, uint64_t k, uint64_t x_rows, const void* const* x_cols,
                      bsm_csr** out);
/* Csr::mul_vector (sparse.rs:468-482): out[i] = sum over row i of
 * v * rhs[col] in ascending column order, dense output, no zero skip. */
int bsm_csr_mul_vector(const bsm_csr* a, const void* rhs, uint64_t rhs_len, void* out,
                       uint64_t out_len);
/* Csr::transpose (sparse.rs:296-318): stable CSR -> CSC. 0 columns ->
 * BSM_ERR_PANIC (the result's finalise panics "big eek", sparse.rs:209-211). */
int bsm_csr_transpose(const bsm_csr* a, bsm_csr** out);
/* Csr::add_sparse (sparse.rs:484-540) / Csr::sub_sparse (sparse.rs:542-599):
 * the reference's per-row two-pointer merge over the operands' entries in
 * storage order (rhs-only entries of sub become T::default() - v), zero
 * results dropped. Dims differ -> BSM_ERR_DIMENSIONS; 0 rows -> BSM_ERR_PANIC
 * (the reference's row loop never ends). Same dtype required. */
int bsm_csr_add_sparse(const bsm_csr* a, const bsm_csr* b, bsm_csr** out);
int bsm_csr_sub_sparse(const bsm_csr* a, const bsm_csr* b, bsm_csr** out);
/* Csr::mul_sparse (sparse.rs:601-635): dims (a.rows, b.cols), no dimension
 * check; every result entry is the reference's merge of a's row (storage
 * order) with row j of b.transpose(), kept when nonzero. */
int bsm_csr_mul_sparse(const bsm_csr* a, const bsm_csr* b, bsm_csr** out);
/* impl Csr<f32>::cholesky_decomp (sparse.rs:682-714); F64 is this build's
 * addition. Square check -> BSM_ERR_NON_SQUARE.
 * Non-SPD inputs store the reference's NaN/inf, unsorted rows are read as
 * get_row_complete does, the :707 unwrap on an unregistered L row ->
 * BSM_ERR_PANIC; those (and bands > 1073) need n <= 16384, else
 * BSM_ERR_UNSUPPORTED. bsm_solve follows the same rules. */
int bsm_csr_cholesky(const bsm_csr* a, bsm_csr** out);
/* forward_substitution (lib.rs:28-46): solve L y = b for k RHS columns of n. */
int bsm_forward_substitution(const bsm_csr* l, uint64_t k, uint64_t n,
                             const void* const* b_cols, void* const* y_cols);
/* backward_substitution (lib.rs:49-65): solve U x = y, U = L^T as a Csr. */
int bsm_backward_substitution(const bsm_csr* u, uint64_t k, uint64_t n,
                              const void* const* y_cols, void* const* x_cols);
/* solve (lib.rs:11-24): x = A^-1 b via cholesky_decomp + transpose +
 * forward/backward substitution, all on the device. */
int bsm_solve(const bsm_csr* a, uint64_t k, uint64_t n, const void* const* b_cols,
              void* const* x_cols);
/* solve (lib.rs:11-24) with the triangular solves REASSOCIATED: 64-row
 * blocks, precomputed inverse diagonal blocks, far sums in any order. The
 * factor is the reference-order one; x is NOT bit-exact with the reference but
 * within its f64 tolerance (1e-6 relative, BASELINE.json north_star). Same
 * arguments, errors and panics as bsm_solve. This build's addition. */
int bsm_solve_blocked(const bsm_csr* a, uint64_t k, uint64_t n, const void* const* b_cols,
                      void* const* x_cols);
/* solve (lib.rs:11-24) by a nested-dissection multifrontal Cholesky of
 * P A P^T: P from recursive BFS level-set bisection of A's graph (host), the
 * separator tree's dense fronts factored level by level on the device. x is
 * NOT bit-exact with the reference (another elimination order) but within its
 * f64 tolerance (1e-6 relative, BASELINE.json north_star). A is its lower
 * triangle (j <= i) mirrored, as cholesky_decomp reads it; rows must have
 * strictly increasing columns, and a pivot <= 0 (not SPD) -> BSM_ERR_UNSUPPORTED.
 * Same arguments and panics as bsm_solve. This build's addition.
 * Plans: the analysis of a pattern (ordering, tree, device index arrays) is
 * kept on the handle AND in a library-wide cache keyed by the pattern (a
 * 128-bit device hash of row_ptr and col, each hit confirmed by comparing
 * the pattern itself), because solve takes `a` by value (lib.rs:11) and a
 * drop-in caller uploads a new handle for every call: a new handle with a
 * pattern seen before skips the analysis. Retention: after a solve the plan
 * keeps its numeric storage (the fronts, inverse diagonal tiles and flags:
 * ~5.6 GB at C5 in f64) for the next solve of that pattern. The cache holds
 * at most BSM_ND_CACHE_ENTRIES patterns (default 4, least recently used
 * out) and at most BSM_ND_CACHE_MB of kept storage (default 32768) across
 * them; an allocation that fails for lack of memory first drops the other
 * plans' kept storage and retries. bsm_nd_cache_clear releases every cached
 * plan not also held by a live handle (bsm_csr_free releases the handle's).
 * Env BSM_ND_CACHE=0: no plan kept anywhere; BSM_ND_SHARED=0: per handle only;
 * BSM_ND_KEEP=0: numeric storage freed after every solve. A plan also holds
 * A's lower entries sorted by front tile (8 bytes each) and two small
 * per-task arrays. With one right-hand side (k == 1) the forward solve is
 * formed inside the factor (another summation order than k > 1, within
 * rounding; BSM_ND_FOLD=0 turns it off). Two pipelines: the default one
 * (each factor tile stages its entries of A and pulls its children's update
 * blocks itself) and, with BSM_ND_PLAIN=1, the plain one (fronts zeroed, A
 * assembled, one extend-add launch per level, the forward solve always its
 * own pass): the same factor bits, and the same x except that k == 1 is not
 * folded. A pattern with nnz >= 2^31 takes the plain pipeline by itself
 * (the default one's per-tile offsets are 32-bit), so there x for k == 1
 * differs from the folded form in the last bits (within 1e-12 relative, the
 * BSM_ND_FOLD tolerance); no test can run that size. The other switches
 * (README.md's table) change no bits. */
int bsm_solve_nd(const bsm_csr* a, uint64_t k, uint64_t n, const void* const* b_cols,
                 void* const* x_cols);
/* The factor of bsm_solve_nd, kept: factor once, solve many times, export L.
 * This build's addition; the reference's counterpart is cholesky_decomp
 * (sparse.rs:682-714) returning L for forward_substitution /
 * backward_substitution (lib.rs:28-65).
 *  - bsm_nd_factor_create: the analysis (through the plan caches above) and
 *    the numeric factor of P A P^T. Arguments, preconditions and errors are
 *    bsm_solve_nd's (square, f32/f64, n < 2^31, strictly increasing columns;
 *    not positive definite -> BSM_ERR_UNSUPPORTED, reported here and not at
 *    the first solve). No right-hand side is involved, so nothing is folded;
 *    the factor's bits are those of bsm_solve_nd's. n == 0 gives a valid
 *    empty factor.
 *    Retention: the handle shares the pattern's plan (it survives
 *    bsm_csr_free(a) and bsm_nd_cache_clear) but OWNS its numeric storage, the
 *    fronts and the inverse diagonal tiles (~5.6 GB at C5 in f64): not the
 *    plan's kept storage, which the next bsm_solve_nd of the pattern
 *    overwrites. That memory is outside the BSM_ND_CACHE_MB budget, is never
 *    dropped by the cache's trimming, is reported by bsm_nd_factor_info
 *    (*bytes) and lives until bsm_nd_factor_free.
 *  - bsm_nd_factor_solve: x = A^-1 b on the kept factor for k >= 0 columns
 *    (host buffers, synchronous, as bsm_solve_nd): only the gather, the
 *    forward levels (always the separate pass, for k == 1 too), the backward
 *    levels and the scatter. Column j of x does not depend on k, and equals
 *    bsm_solve_nd's column bit for bit (for k == 1: bsm_solve_nd with
 *    BSM_ND_FOLD=0). n != rows -> BSM_ERR_PANIC. Solves on one handle from
 *    several threads run one after the other.
 *  - bsm_nd_factor_info: rows, dtype, device bytes the handle owns, and the
 *    stored entries of L (0 until an export has counted them). Any pointer
 *    may be NULL.
 *  - bsm_nd_factor_perm: P as n entries, perm[new] = old (bsm_nd_analyse's
 *    convention): (P A P^T)[i][j] = A[perm[i]][perm[j]].
 *  - bsm_nd_factor_export: the factor as ordinary device Csr handles (either
 *    pointer may be NULL; free them with bsm_csr_free), n x n in the NEW
 *    order. *l_star = L^T: row j is column j of L, ascending, the diagonal
 *    entry FIRST (what backward_substitution reads, lib.rs:49-65). *l = L:
 *    rows ascending, the diagonal LAST (forward_substitution, lib.rs:28-46,
 *    and cholesky_decomp's output convention); it is bsm_csr_transpose of
 *    *l_star. Entries that are exactly zero are not stored (insert's rule,
 *    sparse.rs:229); every row keeps its positive diagonal. L L^T = P A P^T
 *    up to rounding. L with 2^32 or more entries -> BSM_ERR_UNSUPPORTED (the
 *    transpose's limit).
 *  - bsm_nd_factor_refactor: new values on the same pattern (Newton steps,
 *    time stepping): the numeric factor alone, on the handle's plan and into
 *    its own storage; no analysis, no cache lookup, no allocation of fronts.
 *    The plan was fixed at create time: BSM_ND_LEAF / _PLAIN / _LAG are not
 *    read again. `a` must be the factored matrix with other values: same
 *    device, dtype, n, nnz, row_ptr and col, which the factor checks itself
 *    against the device copy of the pattern it keeps (the plan cache may be
 *    off or cleared). Any difference -> BSM_ERR_INVALID naming the field, the
 *    factor untouched. On success the factor is, bit for bit, what
 *    bsm_nd_factor_create(a) gives, and nnz_l is 0 again. Values that are not
 *    positive definite -> BSM_ERR_UNSUPPORTED (a hand-off timeout ->
 *    BSM_ERR_HIP); the old factor is overwritten by then, so the handle holds
 *    NO factor: solve, solve_system, the device solve, export and logdet
 *    return BSM_ERR_INVALID ("factor holds no values; refactor first") until
 *    a later refactor succeeds; info, perm and free keep working. n == 0:
 *    BSM_OK, nothing done. Solves and exports on other threads run before or
 *    after a refactorisation, never during it.
 *    The pattern copy (8 (n + 1) + 4 nnz bytes, 28 MB at C5) is shared by the
 *    plan cache's entry and every factor of the plan, and freed with the last
 *    of them; bsm_nd_factor_info's *bytes does NOT count it.
 *  - bsm_nd_factor_logdet: log det A = 2 sum log L_qq over the n pivots,
 *    summed in f64 (for f32 too) in a fixed order that depends on n alone:
 *    the same bits on every call and device. Synchronous. n == 0 -> 0.0.
 *  - bsm_nd_factor_solve_system: bsm_nd_factor_solve's arguments and errors,
 *    plus the system. BSM_ND_SYS_A: bsm_nd_factor_solve itself. BSM_ND_SYS_L:
 *    L y = b, the forward levels alone; BSM_ND_SYS_LT: L^T x = y, the backward
 *    levels alone. For L and LT, b, y and x are in the NEW order (the order
 *    of bsm_nd_factor_export and bsm_nd_factor_perm; nothing is permuted),
 *    so x = P^T LT(L(P b)) has the bits of BSM_ND_SYS_A's x. Another system
 *    value -> BSM_ERR_INVALID.
 *  - bsm_dev_nd_factor_solve: the same solve with b and x in HBM on the
 *    factor's device, ROW-major n x k (bsm_dev_spmm's X and Y), on `stream`;
 *    x == b is allowed. No host copy of b or x and no allocation beyond the
 *    calling thread's cached solve temporaries. It returns after the status
 *    word is read back: synchronous for that stream. The same kernels, hence
 *    the same bits, as the host call. A null pointer with n k > 0 ->
 *    BSM_ERR_INVALID.
 *  - bsm_nd_factor_selinv: the selected inverse, Z = A^-1 on the pattern of
 *    L + L^T (the marginal variances and neighbour covariances of a Gaussian
 *    with precision A), by the Takahashi recursion over the factor's fronts:
 *    a few times the factor's own flops instead of n solves. diag: n values,
 *    diag[i] = Z[i][i] in A's order, or NULL. vals[e] = Z[rows[e]][cols[e]]
 *    for e < nq, indices in A's order, either triangle ((i, j) and (j, i)
 *    give the same bits); rows / cols / vals may be NULL when nq == 0. Host
 *    buffers, diag and vals of the factor's dtype. Errors: a null f,
 *    diag == NULL with nq == 0, or a null among rows / cols / vals with
 *    nq > 0 -> BSM_ERR_INVALID ("null ..."), before any device is asked for;
 *    an index >= n -> BSM_ERR_OUT_OF_BOUNDS; a pair outside the pattern of
 *    L + L^T (every stored entry of A is inside it) -> BSM_ERR_INVALID naming
 *    how many pairs and the first one; a handle without values (a failed
 *    refactor) -> BSM_ERR_INVALID as for the solves. On every error diag and
 *    vals are untouched. The call allocates Z (a second set of fronts: 8
 *    bytes x the factor's front elements, 5.98 GB at C5 in f64) and a 64-wide
 *    panel per front, and frees them before it returns; they are not part of
 *    bsm_nd_factor_info's *bytes nor of the plan cache's budget. The factor is
 *    only read. Every sum has a fixed order: the same bits on every call.
 *    Synchronous; other calls on the handle run before or after it.
 *  - bsm_dev_nd_factor_inv_diag: the diagonal alone into HBM on the factor's
 *    device (n values of its dtype), on `stream`; returns after the stream has
 *    drained. The same kernels and bits as bsm_nd_factor_selinv's diag. A null
 *    f, or a null diag with n > 0 -> BSM_ERR_INVALID.
 *  - bsm_nd_factor_create_as: bsm_nd_factor_create with the factor's dtype
 *    chosen: factor_dtype is BSM_F64 or BSM_F32 (anything else ->
 *    BSM_ERR_INVALID, before any device is asked for). Equal to a's dtype it
 *    IS bsm_nd_factor_create. Otherwise a's values are converted once
 *    (round-to-nearest) into a temporary of the factor's dtype and the same
 *    numeric path runs on them: the f32 factor of an f64 matrix has the bits
 *    of bsm_nd_factor_create on that matrix rounded to f32, and half the f64
 *    factor's bsm_nd_factor_info bytes. The plan and the caches know no dtype
 *    and are shared as ever. bsm_nd_factor_info reports the FACTOR's dtype,
 *    in which solve, solve_system, export, logdet and selinv work; the handle
 *    remembers the matrix's, which bsm_nd_factor_refactor's matrix must have
 *    (it is converted the same way).
 *  - bsm_nd_factor_solve_refined: iterative refinement on the kept factor
 *    (what xPORFS / DSPOSV do): x_0 = M^-1 b by the factor, then corrections
 *    x += M^-1 r from residuals r = b - S x formed in f64, for each of the k
 *    columns on its own. `a` is the system's matrix, n x n on f's device, f32
 *    or f64; b_cols / x_cols are host columns of a's dtype; f may have either
 *    dtype. The system solved is S x = b with S[i][j] = A[max(i,j)][min(i,j)]
 *    over a's stored entries with column <= row: the matrix the factor reads
 *    (entries above the diagonal are ignored). `a` is not compared with the
 *    factored matrix: it may be a nearby one (a stale factor), and the loop
 *    then converges as fast as M^-1 S is close to I. The backward error
 *      omega_j = ||r_j||inf / (||S||inf ||x_j||inf + ||b_j||inf)
 *    is computed after every solve; a column goes on while omega_j > tol and
 *    omega_j <= half the one before (LAPACK's stagnation rule), for at most
 *    max_iter corrections; x_j is the iterate with the smallest omega_j, which
 *    berr[j] reports, after iters[j] corrections (both host arrays of k, or
 *    NULL). tol == 0: the default (m + 2) 2^-53, m the longest row of S, the
 *    rounding bound of the f64 residual itself; tol < 0 or NaN ->
 *    BSM_ERR_INVALID. Right-hand sides and residuals are scaled by a power of
 *    two into [1, 2) before they are cast to the factor's dtype (exact, so a
 *    residual of 1e-13 ||b|| stays normal in f32). b_j == 0 gives x_j = 0,
 *    berr 0, iters 0; a non-finite omega stops its column. BSM_OK whether or
 *    not the columns converged: berr[j] <= tol says so. Column j's x, iters
 *    and berr depend neither on k nor on the other columns, and the same call
 *    gives the same bits (fixed summation order, no floating-point atomics);
 *    with max_iter == 0 and a's dtype the factor's, x has the bits of
 *    bsm_nd_factor_solve. Errors, all before any device work and with every
 *    output untouched: a null f or a, or a null among b / x with n k > 0 ->
 *    BSM_ERR_INVALID ("null ..."); a not f32 / f64, or on another device ->
 *    BSM_ERR_INVALID; a not n x n -> BSM_ERR_DIMENSIONS; n != rows ->
 *    BSM_ERR_PANIC as bsm_nd_factor_solve; a handle without values ->
 *    BSM_ERR_INVALID as for the solves. S is built on the first call and kept
 *    on `a` until bsm_csr_free (row_ptr int64, columns int32, values of a's
 *    dtype: about a's own size).
 *  - bsm_dev_nd_factor_solve_refined: the same with b and x in HBM on the
 *    factor's device, ROW-major n x k of a's dtype (x may be b), on `stream`;
 *    synchronous for that stream. The same kernels and bits as the host call.
 *  - bsm_nd_factor_solve_pcg: preconditioned conjugate gradients on the kept
 *    factor, for the systems refinement cannot do: S x = b as above with M^-1
 *    the factor's solve as preconditioner, each of the k columns its own CG.
 *    It converges for any positive definite S and M (a stale factor, the
 *    factor of a scaled or low-rank-changed matrix), where the refined solve
 *    needs rho(I - M^-1 S) < 1. Arguments as bsm_nd_factor_solve_refined's;
 *    everything but M^-1 is f64 for both dtypes of a. x_0 = M^-1 b is the
 *    refined solve's first iterate (max_iter == 0 gives the bits of
 *    bsm_nd_factor_solve_refined with max_iter == 0 in x and berr). Then at
 *    most max_iter steps (50 is the usual choice): q = S p, alpha = rho /
 *    (p . q), x += alpha p, r -= alpha q, z = M^-1 r (r scaled by a power of
 *    two into [1, 2) and cast to the factor's dtype), beta = -alpha (q . z) /
 *    rho (the flexible form: an M^-1 rounded to f32 and rescaled per step is
 *    not one linear operator), rho = r . z, p = z + beta p. omega_j of the
 *    recurrence's r is computed after every step; at or below tol the true
 *    residual b - S x is formed: at or below tol too the column has
 *    converged, otherwise it takes the true residual for r and goes on with
 *    beta = 0 (a restart). iters[j] counts the steps, berr[j] is the omega of
 *    the TRUE residual of the returned x_j, tol and its default are the
 *    refined solve's. flags (uint32 [k] or NULL): bit 0 set where the column
 *    broke down -- p . q or r . z was <= 0 or not finite, so S or the factor
 *    is not positive definite -- and stopped with the x of its last completed
 *    step. A non-finite omega stops its column; b_j == 0 gives x_j = 0, berr
 *    0, iters 0. BSM_OK in all these cases: berr[j] <= tol says whether
 *    column j converged. Column j's x, iters, berr and flags depend neither
 *    on k nor on the other columns, and the same call gives the same bits
 *    (sums of a fixed number of partials in a fixed order, no floating-point
 *    atomics). Errors and their codes are bsm_nd_factor_solve_refined's, all
 *    before any device work and with every output untouched. Temporaries: six
 *    f64 n x k arrays and one of the factor's dtype.
 *  - bsm_dev_nd_factor_solve_pcg: the same with b and x in HBM on the
 *    factor's device, ROW-major n x k of a's dtype (x may be b), on `stream`;
 *    synchronous for that stream. The same kernels and bits as the host call.
 *  - bsm_nd_factor_eigsh: the nev smallest eigenvalues of S (as above: a's
 *    lower triangle mirrored) and their eigenvectors, by block shift-invert
 *    Lanczos at sigma = 0: the operator is A^-1, which the factor makes cheap,
 *    and its largest eigenvalues theta are the wanted 1 / lambda. The basis is
 *    kept as blocks V_0, V_1, ... of `block` columns (1..32), at most ncv
 *    columns (rounded down to a multiple of block; 0: min(n, 128)). V_0 is
 *    v0_cols (block host columns of a's dtype) or, for NULL, bsm_hash(seed,
 *    row, column, 6) through bsm_unit_uniform mapped to [-1, 1) and rounded to
 *    a's dtype, orthonormalised like every later block. A step is W = A^-1
 *    V_j by bsm_nd_factor_solve_refined's loop (max_iter 5, its default tol,
 *    the block passed in a's dtype: f64 backward error for an f64 a whichever
 *    dtype the factor has, f32 operator accuracy for an f32 a); classical
 *    Gram-Schmidt twice against every block so far (C = V^T W, W -= V C; A_j
 *    is the symmetrised block of the summed C that belongs to V_j); Cholesky-
 *    QR twice (W^T W = R1^T R1, W = W R1^-1, again with R2; V_{j+1} = W,
 *    B_{j+1} = R2 R1). A pivot of the first Cholesky <= 2^-50 times the
 *    column's squared norm before the projections means the block has lost
 *    rank: the Krylov space is invariant, the run stops (info flag bit 0,
 *    "exhausted") and returns the pairs of the basis so far, fewer than nev
 *    where the basis is smaller (lam and resid NaN, vectors 0 for the rest).
 *    The host solves T s = theta s for the block-tridiagonal T of the A_j
 *    and B_j (cyclic Jacobi, no LAPACK) after every step that has nev
 *    columns; est_i = ||B_{j+1} s_i[last block rows]||2 / |theta_i|, and the
 *    run stops when the nev largest theta all have est <= tol, or at ncv.
 *    tol == 0: 2^-26 for an f64 a, 2^-12 for an f32 a (the square root of the
 *    unit roundoff: the eigenvalue error is quadratic in the residual, so the
 *    values are good to the roundoff over the relative gap; pass a smaller
 *    tol for sharper vectors). Results: lam[nev] ascending, vec_cols (nev host
 *    columns of a's dtype, or NULL for values only) of unit 2-norm without a
 *    sign convention, resid[i] = ||S y_i - lam_i y_i||2 / ||y_i||2 formed anew
 *    in f64 from the f64 vectors; since S y - lam y = -lam S (A^-1 y - theta
 *    y), a pair with est <= tol has resid <= tol ||S||inf up to rounding.
 *    info (uint32 [4] or NULL): the steps, the basis columns used, the pairs
 *    with est <= tol, flags (bit 0 exhausted; bit 1 "inexact": a solve's
 *    backward error ended above the refined solve's tol, and the run went
 *    on). BSM_OK whether or not the pairs converged: info and resid say. There
 *    is no restart: call again with v0 = the first `block` vectors returned
 *    and a larger ncv. An eigenvalue of multiplicity above `block` is found
 *    `block` times at most (in exact arithmetic: a run that goes on long after
 *    those copies have converged may pick up a further one from rounding; do
 *    not count on it). The same call gives the same bits (per-workgroup
 *    partials whose number and order depend on n and block alone, or on S,
 *    added in index order; no floating-point atomics). Errors, all before any
 *    device work and with every output untouched: a null f, a, lam or resid ->
 *    BSM_ERR_INVALID ("null ..."); tol < 0 or NaN, nev < 1, block outside
 *    1..32, ncv (after rounding) < nev or > n -> BSM_ERR_INVALID naming the
 *    argument; dtype, device, dimensions and a handle without values as
 *    bsm_nd_factor_solve_refined. n == 0 is accepted with nev == 0. An ncv
 *    above 8192 -> BSM_ERR_UNSUPPORTED (T is dense on the host).
 *    Temporaries: (ncv + 3 block) n f64 and the partials, plus the refined
 *    solve's for `block` columns.
 *  - bsm_dev_nd_factor_eigsh: the same with v0 and the vectors in HBM on the
 *    factor's device, ROW-major n x block and n x nev of a's dtype (either may
 *    be NULL), on `stream`; synchronous for that stream. The same kernels and
 *    bits as the host call.
 *  - bsm_nd_factor_eigsh_gen: the generalised problem S y = lambda S_M y with
 *    a mass matrix m (finite elements and volumes: K x = lambda M x): the nev
 *    smallest lambda, ascending. S_M is m's lower triangle mirrored, exactly as
 *    S is a's (entries above the diagonal are ignored; the copy is kept on m's
 *    handle); m is an n x n bsm_csr of a's dtype on the factor's device with
 *    any pattern. m == NULL calls bsm_nd_factor_eigsh: the same bits. S_M must
 *    be positive definite; a singular mass matrix (constraints, massless
 *    degrees of freedom), a shift sigma != 0 and restarts are out of scope.
 *    The loop is bsm_nd_factor_eigsh's in the S_M inner product, in which the
 *    operator A^-1 S_M is self-adjoint: every block is made S_M-orthonormal;
 *    a step is W = A^-1 (S_M V_j) by the same refined solve; norm2_c = w_c^T
 *    S_M w_c; classical Gram-Schmidt twice with C = V^T (S_M W), W -= V C;
 *    Cholesky-QR twice on G = W^T S_M W with the same rank rule; B_{j+1} = R2
 *    R1. Since S_M (W R^-1) = (S_M W) R^-1, W and S_M W go through the two
 *    W R^-1 passes together and the step ends with S_M V_{j+1} for the next
 *    one: three products with S_M per step (after the solve and after each
 *    projection pass) and one for the start block; S_M V is not kept for the
 *    basis. T, the Ritz solve, est, the stop rule, lambda = 1 / theta, info and
 *    the flags are bsm_nd_factor_eigsh's. The vectors are normalised to y^T
 *    S_M y = 1, without a sign convention, and rounded to f32 for an f32 a.
 *    resid[i] = ||S y_i - lam_i S_M y_i||2 / ||y_i||2, formed anew in f64 from
 *    the vectors as they are returned (with S_M = I: bsm_nd_factor_eigsh's).
 *    With e = A^-1 S_M y - theta y, S y - lam S_M y = -lam S e and ||e||_M =
 *    est theta ||y||_M, so a pair with est <= tol has resid <= tol ||S||inf
 *    sqrt(mu_max / mu_min) up to rounding, mu the extreme eigenvalues of S_M:
 *    the loop stops on est, and an ill-conditioned m may need a smaller tol
 *    for a wanted residual. Errors, all before any device work and with every
 *    output untouched: bsm_nd_factor_eigsh's; m not f32/f64 -> BSM_ERR_INVALID;
 *    m's dtype not a's -> BSM_ERR_INVALID; m on another device ->
 *    BSM_ERR_INVALID; m not n x n -> BSM_ERR_DIMENSIONS. A norm2_c that is <=
 *    0 or not finite (of the start block or of a step; a zero column of v0
 *    reads the same), or an m without stored entries, means that S_M is not
 *    positive definite: BSM_ERR_UNSUPPORTED ("m is not positive definite"),
 *    as bsm_nd_factor_create reports it for a, every output untouched; an
 *    indefinite S_M that no block exposes ends as "exhausted". Temporaries:
 *    bsm_nd_factor_eigsh's plus one n x block f64 array, (ncv + 4 block) n f64
 *    in all (S_M V_j between the steps and S_M W inside one share it), the
 *    partials and the refined solve's. The same call gives the same bits (the
 *    products with S_M take a row's entries in stored order by a fixed number
 *    of lanes and a fixed xor tree; the partials as above; no floating-point
 *    atomics).
 *  - bsm_dev_nd_factor_eigsh_gen: the same with v0 and the vectors in HBM, as
 *    bsm_dev_nd_factor_eigsh; m == NULL calls that function.
 *  - bsm_nd_factor_updown: the rank-k update (sign = +1) or downdate
 *    (sign = -1) of the kept factor: afterwards f is the factor of
 *    P (S + sign W W^T) P^T, S the matrix it was the factor of. Only the fronts
 *    on the paths from W's columns to the root of the separator tree are
 *    rewritten (14 of 15,397 at C5 for one edge), by the column-by-column method
 *    (Gill, Golub, Murray, Saunders C1), the k columns in column order at every
 *    pivot. W is n x k, column-compressed on the host: col_ptr has k + 1
 *    entries, rows (A's order) is strictly ascending within a column, vals has
 *    the FACTORED MATRIX's dtype (an f32 factor of an f64 matrix rounds them
 *    once). 1 <= k <= 16; larger ranks call again. Which W: with a column's
 *    entry of the smallest new index (bsm_nd_factor_perm) in tree node N,
 *    every other entry must be an own column of N or one of N's front rows.
 *    Always inside: a diagonal column alpha e_i, and a vertex with any of its
 *    neighbours in S's graph that come later in the new order (an edge
 *    sqrt(c) (e_i - e_j) of a stored (i, j); an element's clique seen from its
 *    first vertex). Errors, in this order, all before any device write: a null
 *    f, a null among col_ptr / rows / vals where they are read, a sign that
 *    is neither +1 nor -1, col_ptr not ascending from 0 or rows not strictly
 *    ascending within a column -> BSM_ERR_INVALID; k > 16 ->
 *    BSM_ERR_UNSUPPORTED; a row >= n -> BSM_ERR_OUT_OF_BOUNDS; a handle
 *    without values (a failed refactor) -> BSM_ERR_INVALID as for the solves;
 *    a column outside the pattern -> BSM_ERR_INVALID naming how many columns
 *    and the first one; a downdate that leaves the matrix not positive
 *    definite (found by a dry pass of the same arithmetic that writes only
 *    scratch) -> BSM_ERR_UNSUPPORTED with bsm_nd_factor_create's message, the
 *    factor's bits untouched and the handle still valid. k == 0, empty
 *    columns and stored zeros are no-ops. An update whose values overflow or
 *    are not finite is found while it writes: BSM_ERR_UNSUPPORTED, and the
 *    handle is left without values as after a failed refactor. Afterwards
 *    *nnz_l is 0 again; the solves, logdet, the export, the selected inverse,
 *    the refined and pcg solves and eigsh all see the new factor. The factor's
 *    dtype, explicit fma, no atomics, a fixed order: the same call on the same
 *    factor gives the same bits. Synchronous.
 *  - bsm_nd_factor_solve_sparse: A x = b (A's order) for a SPARSE b, with x
 *    wanted at some rows only (CHOLMOD's Bset / Xset): a Green's function
 *    between two points, an entry or a block of A^-1 off the pattern of
 *    L + L^T. b is n x k, column-compressed on the host as
 *    bsm_nd_factor_updown's W (col_ptr has k + 1 entries, rows strictly
 *    ascending within a column); vals and x have the FACTOR's dtype, as
 *    bsm_nd_factor_solve. xrows: nq rows, unsorted and repeated as the caller
 *    likes, output row e is x[xrows[e]], and x_cols are k host columns of nq
 *    values; xrows == NULL (with nq == 0): every row, x_cols are k columns of
 *    n. Only the fronts on the paths from b's entries to the root run the
 *    forward pass (every other front has y = 0), only those from the requested
 *    rows' fronts to the root the backward pass; each of them performs the
 *    dense solve's operations in its order, so every value returned EQUALS
 *    bsm_nd_factor_solve's on the densified b (a zero may differ in sign: a
 *    skipped front's +0 is not added to a -0). The values at a row depend
 *    neither on the other rows asked for nor on the call's other columns, and
 *    repeat bit for bit. With xrows == NULL the backward pass is the dense
 *    solve's own. Columns go in chunks of 32: the temporaries never exceed the
 *    dense solve's for 32 columns. An empty column gives a zero column and
 *    activates nothing; stored zeros are ordinary entries; k == 0 is a no-op
 *    (nothing is written, info included); nq == 0 with a non-NULL xrows is
 *    valid, writes no x and sets info to 0. info (uint32[4] or NULL): the
 *    fronts the forward pass ran on (the union over the columns), the fronts
 *    the backward pass ran on, the fronts in the plan, the column chunks.
 *    Errors, in this order, all before any device write: a null f, a null
 *    among x_cols (or one of its k columns) / col_ptr / rows / vals where it
 *    is read, col_ptr not ascending from 0 or rows not strictly ascending
 *    within a column, nq > 0 with xrows == NULL -> BSM_ERR_INVALID; a row of b
 *    or of xrows >= n -> BSM_ERR_OUT_OF_BOUNDS; another device, a handle
 *    without values (a failed refactor) -> BSM_ERR_INVALID as for the solves.
 *    A refused call leaves x_cols and info as they were. Takes the handle's
 *    mutex, as the solves do. Synchronous.
 *  - bsm_dev_nd_factor_solve_sparse: the same with x in HBM on the factor's
 *    device, ROW-major nq x k (n x k); b and xrows stay on the host. Runs on
 *    `stream`, returns after it has drained.
 *  - bsm_nd_factor_refactor_partial: new values at a FEW places of the
 *    factored pattern (a Newton or contact step in which a few elements
 *    change, a device that switches, a local material change): only the fronts
 *    on the paths from those entries to the roots of the separator tree are
 *    factored again, by refactor's own kernel on refactor's per-tile inputs in
 *    refactor's order. Precondition: f holds the factor of some a0 on its
 *    pattern, made by bsm_nd_factor_create(_as), bsm_nd_factor_refactor or an
 *    earlier partial call, and no bsm_nd_factor_updown has run since. a has
 *    that pattern (checked as bsm_nd_factor_refactor checks it, with its
 *    errors and messages) and equals a0 in every stored entry (i, j), j <= i,
 *    except possibly at the nc positions (rows[e], cols[e]): host arrays, any
 *    order, (j, i) names the same entry as (i, j), repeats allowed. Entries
 *    above the diagonal are not read, as ever. Afterwards f is the factor of a
 *    and every bit of it that anything reads equals what
 *    bsm_nd_factor_refactor(f, a) writes. A changed entry that is NOT named
 *    gives an unspecified factor (bsm_nd_factor_refactor_since finds the
 *    places itself). info (uint64[3] or NULL): the fronts factored again, the
 *    fronts in the plan, the changed entries (nc as named). Errors, all before
 *    any write to the factor: a null f or a, then nc > 0 with a null rows or
 *    cols -> BSM_ERR_INVALID (no device asked for); another device, dtype,
 *    shape, nnz, row_ptr or col -> bsm_nd_factor_refactor's; an index >= n ->
 *    BSM_ERR_OUT_OF_BOUNDS; a handle on which an update or downdate has run
 *    since its last factorisation -> BSM_ERR_UNSUPPORTED (refactor first: the
 *    update blocks the active fronts would pull are stale); a named pair that
 *    is not a stored entry of a -> BSM_ERR_INVALID with their number and the
 *    first one. nc == 0 runs the checks and leaves the factor's bits (info:
 *    0 fronts); n == 0 is a no-op. A pivot <= 0 or not finite met while
 *    writing leaves the handle without values exactly as a failed
 *    bsm_nd_factor_refactor does (BSM_ERR_UNSUPPORTED, its message; a later
 *    bsm_nd_factor_refactor restores it); a handle already without values is
 *    given the full factorisation of a (every front reported), and so is one
 *    on the plain pipeline (BSM_ND_PLAIN=1, or 2^31 stored entries or more),
 *    which assembles into the fronts and cannot restart one. nnz_l reads 0
 *    until the next export. Takes the handle's mutex. Synchronous.
 *  - bsm_nd_factor_refactor_since: the same for callers who cannot name the
 *    places: a_old (the matrix f is the factor of) and a_new, both on f's
 *    pattern, are compared on the device, and every stored entry with
 *    col <= row whose bits differ (so NaN and -0 count) is a changed place.
 *    info[2] is their number. No differing entry: the factor's bits stay.
 *  - bsm_nd_factor_create_schur: bsm_nd_factor_create_as with a Schur set G:
 *    m distinct vertices idx (A's order, any order among themselves) that the
 *    analysis orders LAST, as the separator tree's root front's own columns
 *    (perm[n - m .. n) = sorted idx); under that root is the ordinary tree of
 *    the other vertices I. The handle is a factor like any other, of P A P^T
 *    with this P: every other call works on it unchanged, and the refactor
 *    calls keep the set. Its plan is the handle's alone, never in the plan
 *    caches. m == 0 gives bsm_nd_factor_create_as's factor (no set). Errors,
 *    before any device is asked for: a null a, out or (m > 0) idx, a
 *    factor_dtype that is no float -> BSM_ERR_INVALID; an index >= n, then a
 *    repeated index -> BSM_ERR_INVALID (naming the entry); m > 16384 ->
 *    BSM_ERR_UNSUPPORTED (the root front is dense: (64 ceil(m / 64))^2 values).
 *  - bsm_nd_factor_schur_info: *m and the set as given (idx_out: m entries).
 *    Any pointer may be NULL; m is 0 for a factor made without a set.
 *  - bsm_nd_factor_schur: S = A_GG - A_GI A_II^-1 A_IG into out (host), m x m
 *    of the FACTOR's dtype, column-major with leading dimension ld >= m, rows
 *    and columns in the order idx was given. a is the matrix the handle is
 *    the factor of: its pattern is checked as bsm_nd_factor_refactor checks it
 *    (with its errors); its VALUES are the caller's responsibility, as in
 *    bsm_nd_factor_solve_refined. Entry (i, j) is a's stored lower entry
 *    between the two vertices (converted to the factor's dtype as the factor's
 *    input is; 0 if none) plus the update-block entry the factorisation left
 *    under the root: one addition, in that order, no atomics; S is exactly
 *    symmetric, the same call gives the same bits, and another order of idx
 *    gives the same values permuted. The root's own L is not read.
 *  - bsm_nd_factor_schur_condense: g = b_G - A_GI A_II^-1 b_I for k columns:
 *    b_cols are k host columns of n values, g_cols k host columns of m (the
 *    order of idx), all of the factor's dtype. The solve's forward levels
 *    below the root, then the root's own gather of b and its child's update
 *    vector.
 *  - bsm_nd_factor_schur_expand: x from b and a given x_G (x_gamma_cols: k
 *    host columns of m, the order of idx; x_cols: k columns of n): the same
 *    forward levels, x_G put where the root's backward step leaves its x, the
 *    backward levels below the root, the scatter. STATELESS: it repeats the
 *    forward pass and keeps nothing between the two calls. With x_G the rows
 *    idx of bsm_nd_factor_solve's x it returns that x bit for bit.
 *    With S x_G = g solved by the caller, condense + expand is a solve.
 *  - bsm_dev_nd_factor_schur / _schur_condense / _schur_expand: the same with
 *    out (column-major, ld), b / x (ROW-major n x k) and g / x_gamma (ROW-major
 *    m x k) in HBM on the factor's device; they run on `stream` and return
 *    after it has drained.
 *    The three calls refuse: a null handle or buffer, a factor made without a
 *    set, ld < m -> BSM_ERR_INVALID (no device asked for); another device, a
 *    handle without values -> BSM_ERR_INVALID; a handle on which an update or
 *    downdate has run since its last factorisation -> BSM_ERR_UNSUPPORTED
 *    (refactor first: the update blocks are stale). Both pipelines
 *    (BSM_ND_PLAIN=1 too) leave the update blocks in place and are supported.
 *    They take the handle's mutex. This build's addition.
 * A factor is used on the device it was made on (else BSM_ERR_INVALID). */
typedef struct bsm_nd_factor bsm_nd_factor;
#define BSM_ND_SYS_A 0  /* A x = b (b and x in A's order) */
#define BSM_ND_SYS_L 1  /* L y = b (new order) */
#define BSM_ND_SYS_LT 2 /* L^T x = y (new order) */
int bsm_nd_factor_create(const bsm_csr* a, bsm_nd_factor** out);
int bsm_nd_factor_solve(const bsm_nd_factor* f, uint64_t k, uint64_t n, const void* const* b_cols,
                        void* const* x_cols);
int bsm_nd_factor_info(const bsm_nd_factor* f, uint64_t* n, int* dtype, uint64_t* bytes, uint64_t* nnz_l);
int bsm_nd_factor_perm(const bsm_nd_factor* f, int64_t* perm);
int bsm_nd_factor_export(const bsm_nd_factor* f, bsm_csr** l, bsm_csr** l_star);
int bsm_nd_factor_refactor(bsm_nd_factor* f, const bsm_csr* a);
int bsm_nd_factor_logdet(const bsm_nd_factor* f, double* logdet);
int bsm_nd_factor_solve_system(const bsm_nd_factor* f, int system, uint64_t k, uint64_t n,
                               const void* const* b_cols, void* const* x_cols);
int bsm_dev_nd_factor_solve(const bsm_nd_factor* f, int system, uint64_t k, const void* b, void* x,
                            void* stream);
int bsm_nd_factor_selinv(const bsm_nd_factor* f, void* diag, uint64_t nq, const uint64_t* rows,
                         const uint64_t* cols, void* vals);
int bsm_dev_nd_factor_inv_diag(const bsm_nd_factor* f, void* diag, void* stream);
int bsm_nd_factor_create_as(const bsm_csr* a, int factor_dtype, bsm_nd_factor** out);
int bsm_nd_factor_solve_refined(const bsm_nd_factor* f, const bsm_csr* a, uint64_t k, uint64_t n,
                                const void* const* b_cols, void* const* x_cols, uint32_t max_iter, double tol,
                                uint32_t* iters, double* berr);
int bsm_dev_nd_factor_solve_refined(const bsm_nd_factor* f, const bsm_csr* a, uint64_t k, const void* b, void* x,
                                    uint32_t max_iter, double tol, uint32_t* iters, double* berr, void* stream);
int bsm_nd_factor_solve_pcg(const bsm_nd_factor* f, const bsm_csr* a, uint64_t k, uint64_t n,
                            const void* const* b_cols, void* const* x_cols, uint32_t max_iter, double tol,
                            uint32_t* iters, double* berr, uint32_t* flags);
int bsm_dev_nd_factor_solve_pcg(const bsm_nd_factor* f, const bsm_csr* a, uint64_t k, const void* b, void* x,
                                uint32_t max_iter, double tol, uint32_t* iters, double* berr, uint32_t* flags,
                                void* stream);
int bsm_nd_factor_eigsh(const bsm_nd_factor* f, const bsm_csr* a, uint64_t nev, uint64_t block, uint64_t ncv,
                        double tol, uint64_t seed, const void* const* v0_cols, double* lam, void* const* vec_cols,
                        double* resid, uint32_t* info);
int bsm_dev_nd_factor_eigsh(const bsm_nd_factor* f, const bsm_csr* a, uint64_t nev, uint64_t block, uint64_t ncv,
                            double tol, uint64_t seed, const void* v0, double* lam, void* vecs, double* resid,
                            uint32_t* info, void* stream);
int bsm_nd_factor_eigsh_gen(const bsm_nd_factor* f, const bsm_csr* a, const bsm_csr* m, uint64_t nev, uint64_t block,
                            uint64_t ncv, double tol, uint64_t seed, const void* const* v0_cols, double* lam,
                            void* const* vec_cols, double* resid, uint32_t* info);
int bsm_dev_nd_factor_eigsh_gen(const bsm_nd_factor* f, const bsm_csr* a, const bsm_csr* m, uint64_t nev,
                                uint64_t block, uint64_t ncv, double tol, uint64_t seed, const void* v0, double* lam,
                                void* vecs, double* resid, uint32_t* info, void* stream);
int bsm_nd_factor_updown(bsm_nd_factor* f, int sign, uint64_t k, const uint64_t* col_ptr, const uint64_t* rows,
                         const void* vals);
int bsm_nd_factor_solve_sparse(const bsm_nd_factor* f, uint64_t k, const uint64_t* col_ptr, const uint64_t* rows,
                               const void* vals, uint64_t nq, const uint64_t* xrows, void* const* x_cols,
                               uint32_t* info);
int bsm_dev_nd_factor_solve_sparse(const bsm_nd_factor* f, uint64_t k, const uint64_t* col_ptr, const uint64_t* rows,
                                   const void* vals, uint64_t nq, const uint64_t* xrows, void* x, uint32_t* info,
                                   void* stream);
int bsm_nd_factor_refactor_partial(bsm_nd_factor* f, const bsm_csr* a, uint64_t nc, const uint64_t* rows,
                                   const uint64_t* cols, uint64_t* info);
int bsm_nd_factor_refactor_since(bsm_nd_factor* f, const bsm_csr* a_old, const bsm_csr* a_new, uint64_t* info);
int bsm_nd_factor_create_schur(const bsm_csr* a, int factor_dtype, const uint64_t* idx, uint64_t m,
                               bsm_nd_factor** out);
int bsm_nd_factor_schur_info(const bsm_nd_factor* f, uint64_t* m, uint64_t* idx_out);
int bsm_nd_factor_schur(const bsm_nd_factor* f, const bsm_csr* a, void* out, uint64_t ld);
int bsm_dev_nd_factor_schur(const bsm_nd_factor* f, const bsm_csr* a, void* out, uint64_t ld, void* stream);
int bsm_nd_factor_schur_condense(const bsm_nd_factor* f, const void* const* b_cols, uint64_t k, void* const* g_cols);
int bsm_nd_factor_schur_expand(const bsm_nd_factor* f, const void* const* b_cols, uint64_t k,
                               const void* const* x_gamma_cols, void* const* x_cols);
int bsm_dev_nd_factor_schur_condense(const bsm_nd_factor* f, const void* b, uint64_t k, void* g, void* stream);
int bsm_dev_nd_factor_schur_expand(const bsm_nd_factor* f, const void* b, uint64_t k, const void* x_gamma, void* x,
                                   void* stream);
void bsm_nd_factor_free(bsm_nd_factor* f);
/* The differentiable solve's pieces: everything a gradient of x = S^-1 b or of
 * log det S with respect to the stored values needs, with every operand in HBM
 * on the factor's device and the work on `stream`. "The factored pattern" is
 * the row_ptr / col of the matrix given to bsm_nd_factor_create(_as), which the
 * handle keeps; its entries are counted by bsm_nd_factor_pattern_info. This
 * build's addition.
 *  - bsm_nd_factor_pattern_info: *nnz = the factored pattern's stored entries
 *    (both triangles), *src_dtype = the factored matrix's dtype (the factor's
 *    own is bsm_nd_factor_info's). Either pointer may be NULL. No device use.
 *  - bsm_dev_nd_factor_refactor_values: bsm_nd_factor_refactor without the
 *    matrix handle: nnz device values of `dtype` in the factored pattern's
 *    storage order (entries with col > row are ignored, as ever). No upload and
 *    no pattern comparison. dtype must be the factored matrix's and nnz the
 *    pattern's (else BSM_ERR_INVALID, nothing written); an f32 factor of an f64
 *    matrix converts the values as bsm_nd_factor_refactor does. The factor has
 *    the bits bsm_nd_factor_refactor gives on a matrix with these values, under
 *    either pipeline. Values that are not positive definite: its error, the
 *    handle left without a factor until a later good call. Takes the handle's
 *    mutex; returns after the status word is read.
 *  - bsm_dev_nd_factor_inv_pattern: (S^-1)[i, j] at every stored entry of the
 *    factored pattern, both triangles, nnz values of the FACTOR's dtype in the
 *    pattern's storage order: bsm_nd_factor_selinv's recursion with a read-out
 *    over the kept pattern, the same bits as bsm_nd_factor_selinv on those
 *    pairs. nnz must be the pattern's. Synchronous for `stream`.
 *  - bsm_dev_nd_factor_sddmm: bsm_dev_sddmm (below) in BSM_SDDMM_SYM_LOWER mode
 *    on the factored pattern: u and v are ROW-major n x k of `dtype`, out nnz
 *    values. nnz must be the pattern's. Asynchronous on `stream`.
 * All four refuse a null handle, and a null array with work to do, before any
 * device is asked for. */
int bsm_nd_factor_pattern_info(const bsm_nd_factor* f, uint64_t* nnz, int* src_dtype);
int bsm_dev_nd_factor_refactor_values(bsm_nd_factor* f, int dtype, uint64_t nnz, const void* vals, void* stream);
int bsm_dev_nd_factor_inv_pattern(const bsm_nd_factor* f, uint64_t nnz, void* out, void* stream);
int bsm_dev_nd_factor_sddmm(const bsm_nd_factor* f, int dtype, uint64_t nnz, uint64_t k, const void* u, const void* v,
                            void* out, void* stream);
/* The cross-handle plan cache of bsm_solve_nd: drop every entry, or read its
 * state (entries, kept numeric bytes, lookups that hit / missed since load).
 * Any pointer may be NULL. This build's addition. */
int bsm_nd_cache_clear(void);
int bsm_nd_cache_info(uint64_t* entries, uint64_t* kept_bytes, uint64_t* hits, uint64_t* misses);
/* The analysis of bsm_solve_nd alone, on a host pattern (row_ptr n+1, col_idx
 * row_ptr[n]); no device use (tests, diagnostics). Writes perm (n entries,
 * perm[new] = old) when non-null; *n_nodes and *st_len always; when cap >=
 * *n_nodes and st_cap >= *st_len, the tree in post-order as 8 int64 per node
 * (start, end, parent, level, slot, m, offset into st, 0) and every node's m
 * front rows (new indices, ascending) into st. This build's addition. */
int bsm_nd_analyse(uint64_t n, const uint64_t* row_ptr, const uint64_t* col_idx, uint64_t leaf,
                   int64_t* perm, int64_t* nodes, uint64_t cap, uint64_t* n_nodes, int64_t* st,
                   uint64_t st_cap, uint64_t* st_len);
/* The same with the m distinct vertices `last` ordered last, as the root node's
 * own (bsm_nd_factor_create_schur's analysis): the last node owns [n - m, n),
 * perm[n - m .. n) is `last` sorted, and its one child is the tree of the
 * other vertices. m == 0: bsm_nd_analyse's arrays. An index >= n or a repeated
 * one -> BSM_ERR_INVALID, m > 16384 -> BSM_ERR_UNSUPPORTED. */
int bsm_nd_analyse_last(uint64_t n, const uint64_t* row_ptr, const uint64_t* col_idx, uint64_t leaf,
                        const uint64_t* last, uint64_t m, int64_t* perm, int64_t* nodes, uint64_t cap,
                        uint64_t* n_nodes, int64_t* st, uint64_t st_cap, uint64_t* st_len);

/* ---- device-level entry points (HBM pointers, async on `stream`) --------- */
/* Synthetic CSR generator (bsm_synth.h recipe): rows [row0, row0+rows) of a
 * matrix with n_cols columns, rowlen_kind CONST/UNIFORM (a, b), value_kind
 * UNIFORM/SMALLINT. Writes row_ptr (rows+1, local, starting at 0), col, vals.
 * bsm_dev_gen_row_ptr must run first; its nnz is row_ptr[rows]. Rows longer
 * than 4096 are not supported by the device generator. */
int bsm_dev_gen_row_ptr(uint64_t seed, uint64_t row0, uint64_t rows, uint32_t n_cols,
                        int rowlen_kind, uint32_t a, uint32_t b, int64_t* row_ptr,
                        void* workspace, uint64_t workspace_bytes, void* stream);
int bsm_dev_gen_entries(int dtype, uint64_t seed, uint64_t row0, uint64_t rows,
                        uint32_t n_cols, int value_kind, const int64_t* row_ptr,
                        int32_t* col, void* vals, void* stream);
/* Insert stream shaped like the reference bench (sparse_dense_mul.rs:16-22;
 * bsm_synth.h bsm_stream_draw): entries i0 .. i0+n-1 with row = draw % rows,
 * col = draw % cols, v = draw % vmod (as dtype). Device arrays. */
int bsm_dev_gen_insert_stream(int dtype, uint64_t seed, uint64_t i0, uint64_t n, uint64_t rows,
                              uint64_t cols, uint64_t vmod, uint64_t* row, uint64_t* col, void* vals,
                              void* stream);
/* bsm_csr_from_inserts on device arrays (synchronous on `stream`). */
int bsm_dev_csr_from_inserts(int dtype, uint64_t rows, uint64_t cols, uint64_t n, const uint64_t* row,
                             const uint64_t* col, const void* vals, bsm_csr** out, void* stream);
/* Dense ROW-major n x k operand: X[r][j] = bsm_x_value(seed, row0 + r, j). */
int bsm_dev_gen_dense(int dtype, uint64_t seed, uint64_t row0, uint64_t n, uint64_t k,
                      int value_kind, void* x, void* stream);
/* Workspace bytes needed by the scans of bsm_dev_gen_row_ptr / bsm_dev_spmm_csr. */
uint64_t bsm_dev_scan_workspace_bytes(uint64_t n);
/* Y = A X (dense ROW-major Y, rows x k), the kernel of mul_dense. row_nnz
 * (int32[rows], may be NULL) receives the count of nonzero results per row
 * for compaction. */
int bsm_dev_spmm(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz,
                 const int64_t* row_ptr, const int32_t* col, const void* vals, uint64_t k,
                 const void* x, void* y, int32_t* row_nnz, void* stream);
/* The sampled dense-dense product (SDDMM): out[p] for every stored entry
 * p = (i, j) of a CSR pattern (row_ptr: rows + 1, col: nnz, any column order
 * inside a row), from ROW-major U (rows x k) and V (cols x k) of dtype
 * BSM_F32 / BSM_F64; out has nnz values of it and nothing else is written.
 *   BSM_SDDMM_ALL        out[p] = dot(U[i,:], V[j,:])
 *   BSM_SDDMM_SYM_LOWER  square patterns: j < i: dot(U[i,:], V[j,:]) +
 *                        dot(U[j,:], V[i,:]); j == i: dot(U[i,:], V[i,:]);
 *                        j > i: +0.0
 * dot has one fixed order that depends on k alone (products rounded, no fma;
 * for k <= 64 a halving tree of width the smallest power of two >= k, for
 * k > 64 chunks of 64 columns added in ascending order), so the bits do not
 * depend on the launch, on nnz or on where an entry sits. No atomics.
 * rows == 0 or nnz == 0 launches nothing. k == 0, another dtype or mode, or
 * BSM_SDDMM_SYM_LOWER with rows != cols -> BSM_ERR_INVALID; so is a null
 * array with work to do. This build's addition. */
#define BSM_SDDMM_ALL 0
#define BSM_SDDMM_SYM_LOWER 1
int bsm_dev_sddmm(int dtype, int mode, uint64_t rows, uint64_t cols, uint64_t nnz, const int64_t* row_ptr,
                  const int32_t* col, uint64_t k, const void* u, const void* v, void* out, void* stream);
/* Which kernel bsm_dev_spmm launches for these arguments under the
 * environment as it is now (BSM_SPMV_VARIANT, BSM_SPMV_ITEMS,
 * BSM_SPMM_VARIANT); diagnostic, launches nothing. Only the addresses of x
 * and y are looked at (16-byte alignment). max_row_len: the longest row, or
 * UINT64_MAX when unknown, which is what bsm_dev_spmm itself passes; the
 * handle calls (bsm_csr_mul_dense, bsm_csr_mul_vector) pass the analysed
 * value. Returns 0 for rows == 0 (no launch), -1 for an unknown dtype, else:
 *  1 spmv_thread<12>     2 spmv_wave<8>     3 spmv_wave<12>   4 spmv_wave<16>
 *  5 spmv_rows<16>       6 spmv_stream<2>   7 spmv_stream<4>  8 spmv_stream<8>
 *  9 k32_f64_rows4<4>   10 k32_f64_rows4<2>
 * 11 k32_f64<4>         12 k32_f64<4,pipe> 13 k32_f64<8,pipe>
 * 14 rowwave<2,4>  15 rowwave<4,4>  16 rowwave<8,4>  17 rowwave<16,8>
 * 18 rowwave<32,8> 19 rowwave<64,8>
 * (enum class SpmmKernel, csrc/spmm_rule.hpp). The tiled copy, the column
 * panels and the integer split schedule are chosen before this rule. */
int bsm_dev_spmm_kernel(int dtype, uint64_t rows, uint64_t nnz, uint64_t k, uint64_t max_row_len,
                        const void* x, const void* y);
/* Whether bsm_csr_mul_dense replaces that kernel by the nnz-balanced integer
 * schedule (spmm_split_int) for a matrix of this scalar type and longest row
 * and k right-hand columns, under BSM_SPMM_SPLIT as it is now: the very
 * function the handle path asks. 1 / 0, -1 for an unknown dtype. */
int bsm_dev_spmm_wants_split(int dtype, uint64_t k, uint64_t max_row_len);
/* Width of the column-panel plan bsm_csr_mul_dense has cached for this
 * handle and uses (0 = one pass); diagnostic (see bsm_dev_spmm_plan). */
int bsm_csr_panel_cols(const bsm_csr* m, uint64_t* panel_cols);
/* Column-panel schedule of bsm_dev_spmm for an X larger than the 256 MiB
 * Infinity Cache (DESIGN.md "SpMM: column panels"); same results, bit for
 * bit. bsm_dev_spmm_panel_cols gives the panel width for (dtype, n_cols, k)
 * (0 = one pass is best: the schedule is used for f64, k = 32, X > 1 GiB;
 * env BSM_SPMM_PANEL_COLS overrides). bsm_dev_spmm_plan fills seg
 * (bsm_dev_spmm_plan_bytes bytes) once per matrix, synchronously, and sets
 * *usable = 0 when some row's columns do not visit the panels in order (then
 * call bsm_dev_spmm). bsm_dev_spmm_panelled = bsm_dev_spmm with the plan. */
uint64_t bsm_dev_spmm_panel_cols(int dtype, uint64_t n_cols, uint64_t k);
uint64_t bsm_dev_spmm_plan_bytes(uint64_t rows, uint64_t n_cols, uint64_t panel_cols);
int bsm_dev_spmm_plan(uint64_t rows, uint64_t n_cols, const int64_t* row_ptr, const int32_t* col,
                      uint64_t panel_cols, int32_t* seg, int* usable, void* stream);
int bsm_dev_spmm_panelled(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz,
                          const int64_t* row_ptr, const int32_t* col, const void* vals, uint64_t k,
                          const void* x, void* y, int32_t* row_nnz, uint64_t panel_cols,
                          const int32_t* seg, void* stream);
/* Row-block x column-panel schedule of bsm_dev_spmm (Csr::mul_dense,
 * sparse.rs:426-446) with k = 32 and X beyond the Infinity Cache (the C4
 * shape), or k = 1 and X beyond an XCD's L2 (C2); the copy is built for one k
 * (DESIGN.md "SpMM: row blocks x column panels"). bsm_csr_mul_dense builds
 * it for f64 and f32; these device-level entry points are the f64 form.
 * bsm_dev_tiled_create re-lays the matrix once (12 B per entry, 16 B from
 * 2^24 columns on at k = 32, plus chunk padding: a copy beside the CSR;
 * synchronous on `stream`) and returns BSM_ERR_UNSUPPORTED for a shape it
 * does not serve (cols >= 2^31 at k = 32, >= 2^21 at k = 1; rows so uneven
 * that chunk padding passes 25 % of the entries, unless flags has
 * BSM_TILED_ANY_PADDING) or BSM_ERR_OOM.
 * bsm_dev_spmm_tiled = bsm_dev_spmm on that copy: the same Y and row_nnz,
 * bit for bit (each row still sums in storage order). bsm_dev_tiled_wanted
 * says whether the library would use it for this shape (env BSM_SPMM_TILED:
 * 0 = never, 2 = whenever possible). bsm_tiled_info: bytes of the copy,
 * entry slots (entries + dummies), the panel width in columns, the sweeps
 * per batch of rows (1, or 2: the k = 32 f64 kernel that keeps half-width
 * rows on chip and runs every batch once per half of k) and the rows per
 * wave and batch; any of the out pointers may be NULL.
 * bsm_dev_tiled_half_wanted: whether the copy's model picks the two-sweep
 * kernel for this shape on a device (or stream) of `cus` compute units; env
 * BSM_TILED_HALF=0|1 overrides that choice when a copy is built. */
typedef struct bsm_tiled bsm_tiled;
#define BSM_TILED_ANY_PADDING 1
int bsm_dev_tiled_wanted(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz, uint64_t k,
                         uint64_t max_row_len);
int bsm_dev_tiled_create(uint64_t rows, uint64_t n_cols, uint64_t nnz, const int64_t* row_ptr,
                         const int32_t* col, const double* vals, uint64_t k, int flags,
                         bsm_tiled** out, void* stream);
int bsm_dev_spmm_tiled(const bsm_tiled* t, const double* x, double* y, int32_t* row_nnz,
                       void* stream);
int bsm_dev_tiled_half_wanted(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz, uint64_t k,
                              uint32_t cus);
int bsm_tiled_info(const bsm_tiled* t, uint64_t* bytes, uint64_t* slots, uint64_t* panel_cols,
                   uint32_t* passes, uint32_t* batch_rows);
/* Whether bsm_csr_mul_dense has built (and uses) the tiled copy for this
 * handle; diagnostic. */
int bsm_csr_tiled(const bsm_csr* m, int* in_use);
/* Which route the host transfers of this process took so far; diagnostic.
 * out[0..7]: host-to-device chunks sent direct (pageable DMA) / staged
 * (pinned pipeline), device-to-host chunks direct / staged, result chunks
 * faulted in ahead of the data by host threads, chunk copies that used more
 * than one host thread, bsm_csr_download calls that wrote page-locked
 * destinations directly, bsm_csr_download calls served by the one small
 * pinned buffer. Relaxed process-wide counts; _reset zeroes them. */
int bsm_xfer_counters(uint64_t out[8]);
void bsm_xfer_counters_reset(void);
void bsm_tiled_destroy(bsm_tiled* t);
/* Compaction of a dense result into the reference's output Csr (insert's
 * zero skip, sparse.rs:229): out_row_ptr (rows+1), out_col/out_vals with
 * capacity rows*k. */
int bsm_dev_compact(int dtype, uint64_t rows, uint64_t k, const void* y,
                    const int32_t* row_nnz, int64_t* out_row_ptr, int32_t* out_col,
                    void* out_vals, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- multi-GPU: row blocks + RCCL all-gather (north_star) ----
 * Csr::mul_dense (sparse.rs:426-446) has independent rows (:431-444), so the
 * CSR is cut into P = chunks x world contiguous row blocks ("pieces") of
 * near-equal cost, a row costing its entries plus max(1, nnz/rows) (its output
 * row): bsm_partition_rows. For equal row lengths that is the nnz split; on
 * skewed matrices it keeps every piece under 2*rows/P + 1 rows. Piece
 * c*world + g belongs to global rank g and is computed in round c. Every
 * device keeps a replica of X. The dense Y blocks are assembled on every
 * device by RCCL all-gathers, one per round, in place and issued on a
 * communication stream as soon as the round's SpMM is done, so they overlap
 * the next round's SpMM. The output Csr is compacted on the first local
 * device of each process. Per-row sums do not depend on the partition, so
 * the result is bit-identical to bsm_csr_mul_dense.
 *
 * Two ways to build the context:
 *  - one process drives n_gpus devices (the reference's single-threaded Rust
 *    caller on an 8-GPU node): bsm_multi_create, i.e. SURVEY.md §8b's
 *    bsm_init(int n_gpus) with ncclCommInitAll;
 *  - one process per GPU (bench.py under torch.distributed.run): rank 0 calls
 *    bsm_multi_unique_id, the caller ships the BSM_UNIQUE_ID_BYTES bytes to
 *    every rank, and each rank calls bsm_multi_create_rank (ncclCommInitRank).
 *  - one process per rank with the caller's own transport (no RCCL
 *    communicator): bsm_multi_create_external. bsm_mcsr_step then only runs
 *    this rank's SpMM rounds into its slots of the gathered Y; the caller moves
 *    the slots between ranks (bsm_mcsr_slot_read / _write: slot c*world + r is
 *    round c of rank r, as the all-gather would place it) and calls
 *    bsm_mcsr_compact. bsm_mcsr_mul_dense and bsm_multi_broadcast return
 *    BSM_ERR_UNSUPPORTED on such a context.
 * Every rank of a communicator must make the same collective calls
 * (bsm_mcsr_mul_dense, bsm_mcsr_step, bsm_multi_broadcast) in the same order.
 * Threading: the calls on one bsm_mcsr are serialised by a lock held for the
 * whole call (a mul_dense from several threads on one matrix runs one after
 * the other); different matrices on one context may be driven from different
 * threads only if the context's communicator is not in use by two of them at
 * once (RCCL's rule for a communicator). */
typedef struct bsm_multi bsm_multi;
typedef struct bsm_mcsr bsm_mcsr;
#define BSM_UNIQUE_ID_BYTES 128
int bsm_multi_create(int n_gpus, const int* devices, bsm_multi** out);
int bsm_multi_unique_id(void* id);
int bsm_multi_create_rank(const void* id, int world, int rank, int device, bsm_multi** out);
int bsm_multi_create_external(int world, int rank, int device, bsm_multi** out);
int bsm_multi_is_external(const bsm_multi* ctx, int* external);
/* The piece bounds the multi-GPU path uses (host only, no device needed):
 * bounds[0..pieces] for row_ptr[0..rows]. row_ptr must hold rows + 1 entries
 * (it is not validated against anything: rows is trusted). */
int bsm_partition_rows(const uint64_t* row_ptr, uint64_t rows, uint32_t pieces, uint64_t* bounds);
/* world size, devices driven by this process, global rank of the first one */
int bsm_multi_info(const bsm_multi* ctx, int* world, int* n_local, int* first_rank);
/* Broadcast `bytes` from global rank `root` (its first local device's buffer)
 * into bufs[i] on every local device i (ncclBroadcast; synchronous). */
int bsm_multi_broadcast(bsm_multi* ctx, void* const* bufs, uint64_t bytes, int root);
/* SURVEY.md §8b bsm_finalize: releases streams and communicators. Matrices
 * made on the context must be freed first. */
void bsm_multi_destroy(bsm_multi* ctx);

/* Partitioned upload of a finalised Csr<T> (host arrays, as bsm_csr_upload):
 * each process uploads only its own devices' pieces. chunks >= 1. */
int bsm_mcsr_upload(bsm_multi* ctx, int dtype, uint64_t rows, uint64_t cols, uint64_t nnz,
                    const uint64_t* row_ptr, const uint64_t* col_idx, const void* vals, uint32_t chunks,
                    bsm_mcsr** out);
/* The synthetic matrix of bsm_dev_gen_row_ptr/bsm_dev_gen_entries (seed,
 * row-length family, value family), every device generating only its own
 * pieces (C4's 1e10 entries do not fit a host). */
int bsm_mcsr_generate(bsm_multi* ctx, int dtype, uint64_t seed, uint64_t rows, uint32_t n_cols, int rowlen_kind,
                      uint32_t a, uint32_t b, int value_kind, uint32_t chunks, bsm_mcsr** out);
/* rows, cols, nnz, pieces P, padded piece rows; bounds (P+1 entries, may be NULL) */
int bsm_mcsr_info(const bsm_mcsr* m, uint64_t* rows, uint64_t* cols, uint64_t* nnz, uint32_t* pieces,
                  uint64_t* piece_rows, uint64_t* bounds);
/* Build the per-piece SpMM schedules (schedule: 0 = the library's choice as
 * in bsm_csr_mul_dense, 1 = the row-block x column-panel copy whenever
 * possible, 2 = never the copy) and the gathered-Y and output buffers for k
 * right-hand columns. Synchronous; bsm_mcsr_mul_dense calls it when needed.
 * *plan_ms (may be NULL) receives per-phase host times of the slowest local
 * device: {total, tiled count pass, tiled scan, tiled allocation, tiled
 * write pass, panel plans, buffers}. */
int bsm_mcsr_prepare(bsm_mcsr* m, uint64_t k, int schedule, double* plan_ms);
/* The schedule prepare built, over this process's pieces: how many use the
 * row-block x column-panel copy, its bytes in total, and the panel width in
 * columns (the copy's, else the column-panel plan's; 0 = one pass). */
int bsm_mcsr_plan_info(const bsm_mcsr* m, int* tiled_pieces, int* local_pieces, uint64_t* copy_bytes,
                       uint64_t* panel_cols);
/* Csr::mul_dense on all GPUs: X (k host columns of x_rows, Dense::get_col)
 * uploaded to every local device, the step below, then the output Csr (dims
 * rows x k, zero results dropped, sparse.rs:229) as a new handle on the
 * first local device. x_rows != cols -> BSM_ERR_DIMENSIONS. */
int bsm_mcsr_mul_dense(bsm_mcsr* m, uint64_t k, uint64_t x_rows, const void* const* x_cols, bsm_csr** out);
/* Device level, asynchronous: x_dev[i] = X on local device i (ROW-major
 * cols x k). Enqueues the rounds' SpMMs, the all-gathers of Y and of the
 * per-row nonzero counts, and the compaction; bsm_mcsr_sync waits. */
int bsm_mcsr_step(bsm_mcsr* m, const void* const* x_dev);
int bsm_mcsr_sync(bsm_mcsr* m);
/* HIP-event times of the steps since the last reset on local device i, per
 * step {SpMM rounds (first SpMM start .. last SpMM end on the compute
 * stream), all-gather tail (last SpMM end .. last all-gather end), compaction,
 * whole step}: *n steps, the first min(max, *n) written to ms[4*s ..]. */
int bsm_mcsr_step_times(bsm_mcsr* m, int local, int max, int* n, double* ms);
void bsm_mcsr_reset_times(bsm_mcsr* m);
/* The assembled dense Y (rows x k ROW-major, global row order) and per-row
 * nonzero counts on local device i, copied into caller device buffers
 * (either may be NULL); synchronous. */
int bsm_mcsr_copy_y(const bsm_mcsr* m, int local, void* y, int32_t* row_nnz);
/* The last step's output Csr as a new handle on the local device that
 * compacts it (the first local device, or the output rank's: below). */
int bsm_mcsr_output(const bsm_mcsr* m, bsm_csr** out);
/* Which global rank compacts the gathered Y into the output Csr: -1 (the
 * default) every process (its first local device), r >= 0 only rank r. The
 * other ranks then allocate no output buffers (rows x k x (4 + sizeof(T)) B,
 * 3.84 GB per rank at C4) and skip the compaction; bsm_mcsr_output there
 * returns BSM_ERR_INVALID. Drops a prepared schedule's buffers (call before
 * bsm_mcsr_prepare). Reference: Csr::mul_dense returns one Csr to its one
 * caller (src/sparse.rs:426-446); the row split is this build's. */
int bsm_mcsr_set_output_rank(bsm_mcsr* m, int rank);
/* The compaction of the gathered Y into the output Csr (asynchronous, on the
 * compute stream; bsm_mcsr_step does it itself on a context with a
 * communicator). For an external context, after the slot exchange. */
int bsm_mcsr_compact(bsm_mcsr* m);
/* Slots [first, first + n) of the gathered Y (each piece_rows x k values,
 * ROW-major) and of its per-row nonzero counts (piece_rows int32 each) on local
 * device `local`, to / from caller buffers, host or device (either may be
 * NULL); synchronous. Slot c*world + r holds round c of rank r. */
int bsm_mcsr_slot_read(const bsm_mcsr* m, int local, uint32_t first, uint32_t n, void* y, int32_t* row_nnz);
int bsm_mcsr_slot_write(bsm_mcsr* m, int local, uint32_t first, uint32_t n, const void* y, const int32_t* row_nnz);
void bsm_mcsr_free(bsm_mcsr* m);

#ifdef __cplusplus
}
#endif

#endif /* BSM_H */
