// bsm.hpp -- C++20 host mirror of the reference crate's API
// (jamieapps101/Basic_Sparse_Matrix, src/{sparse,dense,dense_static,util,lib}.rs)
// on top of the C-ABI in bsm.h. Header only; link with -lbsm_hip.
//
// The reference is compiled (Rust) code, so its host side is mirrored in a
// compiled language: same type and method names (`new` -> `new_`, a C++
// keyword), the same argument meaning (Dense::new_default_with_dims takes
// COLUMNS first; Csr::from_data takes ROWS, Dense::from_data COLUMNS) and the
// same error behaviour:
//   * Rust `Result<_, MatErr>`  -> bsm::Result<_> holding a value or a MatErr;
//     `unwrap()` on an Err throws bsm::Panic, as Rust's unwrap panics;
//   * Rust `panic!` (index out of bounds, "big eek", unwrap in solve) ->
//     throws bsm::Panic;
//   * device failures (no GPU, HIP error, out of memory) -> throws
//     bsm::DeviceError. There is no CPU fallback on the hot path.
// Construction and accessors are host logic with the reference's exact
// semantics; mul_dense / mul_dense_s / mul_vector / transpose /
// cholesky_decomp / solve run on the GPU (bit-exact with the reference's
// operation order). A finalised Csr is immutable
// (sparse.rs:223-225), so its device copy is uploaded once and cached; the
// cache is not part of operator== (the derived PartialEq of sparse.rs:68-78).
#ifndef BSM_HPP
#define BSM_HPP

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <optional>
#include <span>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "bsm.h"

namespace bsm {

// ---------------------------------------------------------------- util.rs
/// util.rs:11-34. `MatDim{rows, cols}`; `From<(usize,usize)>` is (rows, cols).
struct MatDim {
    size_t rows = 0, cols = 0;
    MatDim() = default;
    MatDim(size_t r, size_t c) : rows(r), cols(c) {}
    MatDim transpose() const { return {cols, rows}; }
    bool operator==(const MatDim&) const = default;
};

/// util.rs:47-55.
enum class MatErr {
    MatrixFinalised,
    MatrixNotFinalised,
    NonSquareMatrix,
    IncorrectDimensions,
    PaddingSizeSmallerThanOriginal,
    OutOfBounds,
};

inline const char* to_string(MatErr e) {
    switch (e) {
        case MatErr::MatrixFinalised: return "MatrixFinalised";
        case MatErr::MatrixNotFinalised: return "MatrixNotFinalised";
        case MatErr::NonSquareMatrix: return "NonSquareMatrix";
        case MatErr::IncorrectDimensions: return "IncorrectDimensions";
        case MatErr::PaddingSizeSmallerThanOriginal: return "PaddingSizeSmallerThanOriginal";
        case MatErr::OutOfBounds: return "OutOfBounds";
    }
    return "?";
}

/// The reference would `panic!` here.
struct Panic : std::runtime_error {
    using std::runtime_error::runtime_error;
};

/// A device-side failure (no GPU, HIP error, allocation failure): the
/// reference has no such error (MatErr has no device variant).
struct DeviceError : std::runtime_error {
    int code;
    DeviceError(int c, const std::string& msg) : std::runtime_error(msg), code(c) {}
};

/// `Result<T, MatErr>`.
template <class T>
class Result {
public:
    Result(T v) : v_(std::move(v)) {}
    Result(MatErr e) : v_(e) {}
    bool is_ok() const { return v_.index() == 0; }
    bool is_err() const { return !is_ok(); }
    T& unwrap() & {
        check();
        return std::get<0>(v_);
    }
    T unwrap() && {
        check();
        return std::move(std::get<0>(v_));
    }
    MatErr unwrap_err() const {
        if (is_ok()) throw Panic("called `Result::unwrap_err()` on an `Ok` value");
        return std::get<1>(v_);
    }
    bool operator==(MatErr e) const { return is_err() && std::get<1>(v_) == e; }

private:
    void check() const {
        if (is_err())
            throw Panic(std::string("called `Result::unwrap()` on an `Err` value: ") + to_string(std::get<1>(v_)));
    }
    std::variant<T, MatErr> v_;
};

template <>
class Result<void> {
public:
    Result() = default;
    Result(MatErr e) : e_(e) {}
    bool is_ok() const { return !e_; }
    bool is_err() const { return e_.has_value(); }
    void unwrap() const {
        if (e_) throw Panic(std::string("called `Result::unwrap()` on an `Err` value: ") + to_string(*e_));
    }
    MatErr unwrap_err() const {
        if (!e_) throw Panic("called `Result::unwrap_err()` on an `Ok` value");
        return *e_;
    }
    bool operator==(MatErr e) const { return e_ && *e_ == e; }

private:
    std::optional<MatErr> e_;
};

namespace detail {
template <class T> struct dtype_of;
template <> struct dtype_of<double> { static constexpr int value = BSM_F64; };
template <> struct dtype_of<float> { static constexpr int value = BSM_F32; };
template <> struct dtype_of<int32_t> { static constexpr int value = BSM_I32; };
template <> struct dtype_of<uint32_t> { static constexpr int value = BSM_U32; };
template <> struct dtype_of<int64_t> { static constexpr int value = BSM_I64; };
template <> struct dtype_of<uint64_t> { static constexpr int value = BSM_U64; };

template <class T>
concept GpuScalar = requires { dtype_of<T>::value; };

struct HandleFree {
    void operator()(bsm_csr* p) const { bsm_csr_free(p); }
};
using Handle = std::shared_ptr<bsm_csr>;

/// Map a C-ABI status: OK, or an Err the caller returns, or a throw.
inline std::optional<MatErr> status(int rc) {
    switch (rc) {
        case BSM_OK: return std::nullopt;
        case BSM_ERR_DIMENSIONS: return MatErr::IncorrectDimensions;
        case BSM_ERR_NON_SQUARE: return MatErr::NonSquareMatrix;
        case BSM_ERR_OUT_OF_BOUNDS: return MatErr::OutOfBounds;
        case BSM_ERR_PANIC: throw Panic(bsm_last_error());
        default: throw DeviceError(rc, bsm_last_error());
    }
}
inline void check(int rc) {
    if (auto e = status(rc)) throw Panic(std::string("unexpected ") + to_string(*e) + ": " + bsm_last_error());
}

// The process-wide multi-GPU context of mul_dense (the Rust binding's
// OnceLock): gpus = 0 is the single-GPU path.
struct MultiState {
    std::mutex mu;
    bool init = false;
    int gpus = 0;
    uint32_t chunks = 1;
    std::shared_ptr<bsm_multi> ctx;
};
inline MultiState& multi_state() {
    static MultiState st;
    return st;
}
inline void multi_env(MultiState& st) {  // BSM_N_GPUS / BSM_CHUNKS, read once
    if (st.init) return;
    st.init = true;
    if (const char* e = std::getenv("BSM_N_GPUS")) st.gpus = std::atoi(e);
    if (const char* e = std::getenv("BSM_CHUNKS")) st.chunks = (uint32_t)std::max(1, std::atoi(e));
}
/// The context (created on first use) and its chunks, or nullptr for one GPU.
inline std::shared_ptr<bsm_multi> multi_context(uint32_t* chunks) {
    MultiState& st = multi_state();
    std::lock_guard<std::mutex> lk(st.mu);
    multi_env(st);
    if (st.gpus <= 0) return nullptr;
    if (!st.ctx) {
        bsm_multi* c = nullptr;
        if (auto e = status(bsm_multi_create(st.gpus, nullptr, &c)))
            throw Panic(std::string("bsm_multi_create: ") + to_string(*e));
        st.ctx = std::shared_ptr<bsm_multi>(c, [](bsm_multi* p) { bsm_multi_destroy(p); });
    }
    *chunks = st.chunks;
    return st.ctx;
}
/// A matrix partitioned over a context; keeps the context alive.
struct MultiCopy {
    std::shared_ptr<bsm_multi> ctx;
    uint32_t chunks = 1;
    std::shared_ptr<bsm_mcsr> m;
};
}  // namespace detail

/// Route every Csr::mul_dense of this process over n GPUs (row blocks of the
/// CSR on each, RCCL all-gather of the dense result; bit-identical to one
/// GPU); n = 0 returns to the single-GPU path, n = 1 runs the RCCL path on one
/// GPU. chunks: rounds per GPU (an all-gather per round overlaps the next
/// round's SpMM). Env BSM_N_GPUS / BSM_CHUNKS give the default.
inline void set_gpus(int n, uint32_t chunks = 1) {
    detail::MultiState& st = detail::multi_state();
    std::lock_guard<std::mutex> lk(st.mu);
    st.init = true;
    if (n != st.gpus) st.ctx.reset();
    st.gpus = n > 0 ? n : 0;
    st.chunks = chunks ? chunks : 1;
}

// --------------------------------------------------------------- dense.rs
/// dense.rs:4-62: column-major, one vector per column.
template <class T>
class Dense {
public:
    /// dense.rs:13-15 -- COLUMNS first.
    static Dense new_default_with_dims(size_t col_count, size_t row_count) {
        return new_with_dims(T{}, col_count, row_count);
    }
    /// dense.rs:17-19.
    static Dense new_with_dims(T val, size_t col_count, size_t row_count) {
        Dense d;
        d.col_count_ = col_count;
        d.row_count_ = row_count;
        d.data_.assign(col_count, std::vector<T>(row_count, val));
        return d;
    }
    /// dense.rs:21-29: `data` is a list of COLUMNS; row_count = data[0].len().
    static Dense from_data(const std::vector<std::vector<T>>& data) {
        Dense d;
        d.col_count_ = data.size();
        d.row_count_ = data.at(0).size();
        d.data_ = data;
        return d;
    }
    /// dense.rs:31-37.
    std::span<const T> get_col(size_t col_index) const { return data_.at(col_index); }
    std::span<T> get_col_mut(size_t col_index) { return data_.at(col_index); }
    /// dense.rs:40-47.
    MatDim get_dims() const { return {row_count_, col_count_}; }
    bool operator==(const Dense&) const = default;

private:
    size_t col_count_ = 0, row_count_ = 0;
    std::vector<std::vector<T>> data_;
};

// -------------------------------------------------------- dense_static.rs
/// dense_static.rs:4-62: `[[T; ROWS]; COLS]`, column-major.
template <class T, size_t ROWS, size_t COLS>
class DenseS {
public:
    static DenseS new_default() { return new_(T{}); }
    static DenseS new_(T val) {
        DenseS d;
        for (auto& c : d.data_) c.fill(val);
        return d;
    }
    /// dense_static.rs:21-35: `data` is a list of COLUMNS.
    static DenseS from_data(const std::vector<std::vector<T>>& data) {
        DenseS d = new_default();
        for (size_t c = 0; c < COLS; ++c)
            for (size_t r = 0; r < ROWS; ++r) d.data_[c][r] = data.at(c).at(r);
        return d;
    }
    std::span<const T> get_col(size_t col_index) const { return data_.at(col_index); }
    std::span<T> get_col_mut(size_t col_index) { return data_.at(col_index); }
    MatDim get_dims() const { return {ROWS, COLS}; }
    bool operator==(const DenseS&) const = default;

private:
    std::array<std::array<T, ROWS>, COLS> data_{};
};

// -------------------------------------------------------------- sparse.rs
/// sparse.rs:80-91.
template <class T>
struct CsrEntry {
    const T* v;
    size_t col_index;
    size_t row_index;
    bool operator==(const CsrEntry& o) const {
        return *v == *o.v && col_index == o.col_index && row_index == o.row_index;
    }
};

template <class T>
class Csr;

/// sparse.rs:7-33: a COO entry, ordered by row then col.
template <class T>
struct COOEntry {
    size_t row = 0, col = 0;
    T value{};
};

/// sparse.rs:35-54: an unordered entry list with a bounds-checked insert;
/// Csr<T>::from(coo) is `From<COO<T>> for Csr<T>` (sparse.rs:56-66).
template <class T>
class COO {
public:
    static COO with_capacity(MatDim dims, size_t capacity) {
        COO c;
        c.dims_ = dims;
        c.entries_.reserve(capacity);
        return c;
    }
    /// sparse.rs:45-53: Err(OutOfBounds) unless row < rows and col < cols.
    Result<void> insert(COOEntry<T> e) {
        if (dims_.rows <= e.row || dims_.cols <= e.col) return MatErr::OutOfBounds;
        entries_.push_back(e);
        return {};
    }
    const std::vector<COOEntry<T>>& entries() const { return entries_; }
    MatDim dims() const { return dims_; }

private:
    std::vector<COOEntry<T>> entries_;
    MatDim dims_;
};

template <class T>
class Csr {
public:
    // ---------------------------------------------------------- ctors
    /// sparse.rs:117-119.
    static Csr new_(MatDim dims) { return new_with_capacity(dims, 0); }
    /// sparse.rs:121-132.
    static Csr new_with_capacity(MatDim dims, size_t capacity) {
        Csr m;
        m.dims_ = dims;
        m.v_.reserve(capacity);
        m.col_index_.reserve(capacity);
        m.row_index_ = {0};
        return m;
    }
    /// sparse.rs:134-152 (insert_unchecked: a zero `value` IS stored).
    static Result<Csr> eye(MatDim dims, T value) {
        if (dims.cols != dims.rows) return MatErr::IncorrectDimensions;
        Csr m = new_(dims);
        for (size_t n = 0; n < dims.cols; ++n) m.insert_unchecked(value, n, n);
        return std::move(m).finalise();
    }
    /// sparse.rs:154-160.
    static Csr create_diagonal(const std::vector<T>& contents) {
        Csr m = new_({contents.size(), contents.size()});
        for (size_t i = 0; i < contents.size(); ++i) m.insert(contents[i], i, i).unwrap();
        return std::move(m).finalise();
    }
    /// sparse.rs:193-203: `data` is a list of ROWS; zeros are skipped.
    static Csr from_data(const std::vector<std::vector<T>>& data) {
        Csr m = new_({data.size(), data.at(0).size()});
        for (size_t r = 0; r < data.size(); ++r)
            for (size_t c = 0; c < data[r].size(); ++c) m.insert(data[r][c], r, c).unwrap();
        return std::move(m).finalise();
    }
    /// Bulk constructor (this build's addition): adopt a finalised CSR
    /// (row_index has rows + 1 entries).
    static Csr from_csr_arrays(MatDim dims, std::vector<size_t> row_index, std::vector<size_t> col_index,
                               std::vector<T> v) {
        if (row_index.size() != dims.rows + 1) throw std::invalid_argument("row_index must have rows+1 entries");
        Csr m;
        m.dims_ = dims;
        m.row_index_ = std::move(row_index);
        m.col_index_ = std::move(col_index);
        m.v_ = std::move(v);
        m.is_finalised_ = true;
        return m;
    }

    // ------------------------------------------------------- building
    /// sparse.rs:206-219: pad row_index to rows + 1 with nnz ("big eek" when
    /// more rows were registered than the matrix has).
    Csr finalise() && {
        if (!is_finalised_) {
            is_finalised_ = true;
            if (dims_.rows < row_index_.size()) throw Panic("big eek");
            const size_t nnz = v_.size();
            row_index_.resize(dims_.rows, nnz);
            row_index_.push_back(nnz);
        }
        return std::move(*this);
    }
    Csr finalise() const& { return Csr(*this).finalise_copy(); }

    /// sparse.rs:222-233: Err(MatrixFinalised) after finalise; a value equal
    /// to T::default() is silently skipped.
    Result<void> insert(T value, size_t row, size_t col) {
        if (is_finalised_) return MatErr::MatrixFinalised;
        if (!(value == T{})) insert_unchecked(value, row, col);
        return {};
    }

    // ------------------------------------------------------ accessors
    MatDim get_dims() const { return dims_; }
    /// sparse.rs:162-164: the last row_index entry.
    size_t get_nnz() const { return row_index_.empty() ? 0 : row_index_.back(); }
    /// sparse.rs:166-168.
    float get_density() const { return (float)v_.size() / (float)(dims_.rows * dims_.cols); }
    /// sparse.rs:170-180.
    const T* get_val_at(MatDim at) const {
        const size_t s = row_index_.at(at.rows), e = row_index_.at(at.rows + 1);
        for (size_t i = s; i < e; ++i)
            if (col_index_[i] == at.cols) return &v_[i];
        return nullptr;
    }
    /// sparse.rs:252-265 (the last recorded row extends to v.len()).
    std::vector<CsrEntry<T>> get_row_compact(size_t index) const {
        auto [s, e] = row_bounds(index);
        std::vector<CsrEntry<T>> out;
        out.reserve(e - s);
        for (size_t i = s; i < e; ++i) out.push_back({&v_[i], col_index_[i], index});
        return out;
    }
    /// sparse.rs:267-294 (literal expansion, unsorted/duplicate columns included).
    std::optional<std::vector<T>> get_row_complete(size_t index) const {
        if (row_index_.empty() || index >= row_index_.size()) return std::nullopt;
        const size_t s = row_index_[index];
        const size_t e = row_index_.size() == index + 1 ? v_.size() : row_index_[index + 1];
        std::vector<T> out;
        size_t prev = 0;
        for (size_t i = s; i < e; ++i) {
            const size_t c = col_index_[i];
            if (c != 0 && c > prev) out.insert(out.end(), c - prev, T{});
            prev = c + 1;
            out.push_back(v_[i]);
        }
        if (dims_.cols > prev) out.insert(out.end(), dims_.cols - prev, T{});
        return out;
    }
    /// `Iterator for Csr` (sparse.rs:93-114).
    std::optional<CsrEntry<T>> next() {
        if (iter_v_index_ == v_.size()) return std::nullopt;
        while (row_index_[iter_row_index_] == iter_v_index_) ++iter_row_index_;
        CsrEntry<T> e{&v_[iter_v_index_], col_index_[iter_v_index_], iter_row_index_ - 1};
        ++iter_v_index_;
        return e;
    }
    /// sparse.rs:413-416.
    void reset_iter() { iter_row_index_ = iter_v_index_ = 0; }

    const std::vector<T>& v() const { return v_; }
    const std::vector<size_t>& col_index() const { return col_index_; }
    const std::vector<size_t>& row_index() const { return row_index_; }
    bool is_finalised() const { return is_finalised_; }

    // ------------------------------------------------------- hot path
    /// sparse.rs:426-446: self * rhs as a new finalised Csr (rows, rhs.cols),
    /// zero results dropped. GPU (kernels_spmm.hip).
    Result<Csr> mul_dense(const Dense<T>& rhs) const requires detail::GpuScalar<T> {
        if (dims_.cols != rhs.get_dims().rows) return MatErr::IncorrectDimensions;  // :427-429
        std::vector<const void*> cols(rhs.get_dims().cols);
        for (size_t j = 0; j < cols.size(); ++j) cols[j] = rhs.get_col(j).data();
        return mul_cols(cols, rhs.get_dims().rows);
    }
    /// sparse.rs:448-466 (checked against ROWS, :449).
    template <size_t ROWS, size_t COLS>
    Result<Csr> mul_dense_s(const DenseS<T, ROWS, COLS>& rhs) const requires detail::GpuScalar<T> {
        if (dims_.cols != ROWS) return MatErr::IncorrectDimensions;
        std::vector<const void*> cols(COLS);
        for (size_t j = 0; j < COLS; ++j) cols[j] = rhs.get_col(j).data();
        return mul_cols(cols, ROWS);
    }
    /// sparse.rs:468-482: out[i] = sum of row i (ascending columns), written
    /// into the caller's slice.
    Result<void> mul_vector(std::span<const T> rhs, std::span<T> out) const requires detail::GpuScalar<T> {
        if (dims_.cols != rhs.size() || dims_.rows != out.size()) return MatErr::IncorrectDimensions;
        auto h = device();
        if (auto e = detail::status(bsm_csr_mul_vector(h.get(), rhs.data(), rhs.size(), out.data(), out.size())))
            return *e;
        return {};
    }
    /// sparse.rs:296-318 (stable CSR -> CSC on the GPU).
    Csr transpose() const requires detail::GpuScalar<T> {
        if (!is_finalised_ && !v_.empty())
            throw Panic("index out of bounds (transpose of an unfinalised matrix)");
        auto h = device();
        bsm_csr* out = nullptr;
        detail::check(bsm_csr_transpose(h.get(), &out));
        return from_device(detail::Handle(out, detail::HandleFree{}));
    }
    /// sparse.rs:320-323.
    std::pair<Csr, Csr> pair_with_tranpose() && {
        Csr t = transpose();
        return {std::move(*this), std::move(t)};
    }
    /// `impl Csr<f32>::cholesky_decomp` (sparse.rs:682-714); f64 is this
    /// build's addition.
    Result<Csr> cholesky_decomp() const requires std::is_floating_point_v<T> {
        if (dims_.rows != dims_.cols) return MatErr::NonSquareMatrix;  // :683-685
        auto h = device();
        bsm_csr* out = nullptr;
        if (auto e = detail::status(bsm_csr_cholesky(h.get(), &out))) return *e;
        return from_device(detail::Handle(out, detail::HandleFree{}));
    }

    /// sparse.rs:484-540: the per-row merge in storage order, zero sums dropped.
    Result<Csr> add_sparse(const Csr& rhs) const requires detail::GpuScalar<T> {
        if (dims_ != rhs.dims_) return MatErr::IncorrectDimensions;  // :485-487
        return binary(rhs, bsm_csr_add_sparse);
    }
    /// sparse.rs:542-599 (rhs-only entries become T::default() - v).
    Result<Csr> sub_sparse(const Csr& rhs) const requires detail::GpuScalar<T> {
        if (dims_ != rhs.dims_) return MatErr::IncorrectDimensions;  // :543-546
        return binary(rhs, bsm_csr_sub_sparse);
    }
    /// sparse.rs:601-635: dims (rows, rhs.cols), no dimension check.
    Result<Csr> mul_sparse(const Csr& rhs) const requires detail::GpuScalar<T> {
        return binary(rhs, bsm_csr_mul_sparse);
    }
    /// `From<COO<T>> for Csr<T>` (sparse.rs:56-66): stable sort by (row, col),
    /// then the zero-skipping insert sequence and finalise (on the GPU).
    static Csr from(const class COO<T>& coo) requires detail::GpuScalar<T>;

    /// Derived PartialEq over the seven fields of sparse.rs:68-78.
    bool operator==(const Csr& o) const {
        return dims_ == o.dims_ && v_ == o.v_ && col_index_ == o.col_index_ && row_index_ == o.row_index_ &&
               is_finalised_ == o.is_finalised_ && iter_v_index_ == o.iter_v_index_ &&
               iter_row_index_ == o.iter_row_index_;
    }

    /// The device copy (uploaded once per finalised matrix). Rows as the
    /// reference's row loop sees them; panics where it panics.
    detail::Handle device() const {
        if (dev_) return dev_;
        auto [rp, used] = device_row_ptr();
        bsm_csr* h = nullptr;
        static_assert(sizeof(size_t) == sizeof(uint64_t), "usize is 8 bytes (x86_64)");
        detail::check(bsm_csr_upload(detail::dtype_of<T>::value, dims_.rows, dims_.cols, used, rp.data(),
                                     reinterpret_cast<const uint64_t*>(col_index_.data()), v_.data(), &h));
        detail::Handle hd(h, detail::HandleFree{});
        if (is_finalised_) dev_ = hd;
        return hd;
    }

    /// row_ptr (rows + 1) as the reference's row loop sees the matrix, and
    /// the entries it uses; panics where it panics.
    std::pair<std::vector<uint64_t>, size_t> device_row_ptr() const {
        const size_t rows = dims_.rows, nnz = v_.size();
        std::vector<uint64_t> rp(rows + 1);
        if (row_index_.size() >= rows + 1) {
            for (size_t r = 0; r <= rows; ++r) rp[r] = row_index_[r];
            if (row_index_.size() == rows + 1 && !is_finalised_) rp[rows] = nnz;
        } else if (row_index_.size() == rows) {
            for (size_t r = 0; r < rows; ++r) rp[r] = row_index_[r];
            rp[rows] = nnz;
        } else {
            throw Panic("index out of bounds: the len is " + std::to_string(row_index_.size()) +
                        " but the index is " + std::to_string(row_index_.size()));
        }
        for (size_t r = 0; r < rows; ++r)
            if (rp[r + 1] < rp[r]) throw Panic("slice index starts after end");
        const size_t used = rows ? rp[rows] : 0;
        if (used > nnz) throw Panic("slice index starts after end");
        for (size_t i = 0; i < used; ++i)
            if (col_index_[i] >= dims_.cols)
                throw Panic("index out of bounds: column " + std::to_string(col_index_[i]) + " >= " +
                            std::to_string(dims_.cols));
        return {std::move(rp), used};
    }

private:
    Csr() = default;
    Csr finalise_copy() { return std::move(*this).finalise(); }

    /// sparse.rs:237-250: a row is recorded only when it exceeds the running
    /// maximum; an entry for an earlier row is appended to the current last row.
    void insert_unchecked(T value, size_t row, size_t col) {
        dev_.reset();
        mdev_ = {};
        v_.push_back(value);
        col_index_.push_back(col);
        if (row + 1 > row_index_.size()) {
            const size_t start = v_.size() - 1;
            while (row_index_.size() <= row) row_index_.push_back(start);
        }
    }

    std::pair<size_t, size_t> row_bounds(size_t index) const {
        if (index >= row_index_.size())
            throw Panic("index out of bounds: the len is " + std::to_string(row_index_.size()) +
                        " but the index is " + std::to_string(index));
        const size_t s = row_index_[index];
        const size_t e = index == row_index_.size() - 1 ? v_.size() : row_index_[index + 1];
        if (s > e || e > v_.size()) throw Panic("slice index starts after end");
        return {s, e};
    }

    Result<Csr> mul_cols(const std::vector<const void*>& cols, size_t x_rows) const {
        uint32_t chunks = 1;
        if (auto ctx = detail::multi_context(&chunks)) {  // row blocks on every GPU + RCCL all-gather
            auto m = multi_device(ctx, chunks);
            bsm_csr* out = nullptr;
            if (auto e = detail::status(bsm_mcsr_mul_dense(m.get(), cols.size(), x_rows, cols.data(), &out)))
                return *e;
            return from_device(detail::Handle(out, detail::HandleFree{}));
        }
        auto h = device();
        bsm_csr* out = nullptr;
        if (auto e = detail::status(bsm_csr_mul_dense(h.get(), cols.size(), x_rows, cols.data(), &out))) return *e;
        return from_device(detail::Handle(out, detail::HandleFree{}));
    }

    /// The matrix partitioned over the multi-GPU context, cached like the
    /// single-GPU copy for a finalised matrix.
    std::shared_ptr<bsm_mcsr> multi_device(const std::shared_ptr<bsm_multi>& ctx, uint32_t chunks) const {
        if (mdev_.m && mdev_.ctx == ctx && mdev_.chunks == chunks) return mdev_.m;
        auto [rp, used] = device_row_ptr();
        bsm_mcsr* m = nullptr;
        detail::check(bsm_mcsr_upload(ctx.get(), detail::dtype_of<T>::value, dims_.rows, dims_.cols, used, rp.data(),
                                      reinterpret_cast<const uint64_t*>(col_index_.data()), v_.data(), chunks, &m));
        std::shared_ptr<bsm_mcsr> sp(m, [](bsm_mcsr* p) { bsm_mcsr_free(p); });
        if (is_finalised_) mdev_ = {ctx, chunks, sp};
        return sp;
    }

    Result<Csr> binary(const Csr& rhs, int (*fn)(const bsm_csr*, const bsm_csr*, bsm_csr**)) const {
        auto a = device();
        auto b = rhs.device();
        bsm_csr* out = nullptr;
        if (auto e = detail::status(fn(a.get(), b.get(), &out))) return *e;
        return from_device(detail::Handle(out, detail::HandleFree{}));
    }

public:
    static Csr from_device(detail::Handle h) {
        uint64_t rows = 0, cols = 0, nnz = 0;
        int dt = 0;
        detail::check(bsm_csr_shape(h.get(), &rows, &cols, &nnz, &dt));
        Csr m;
        m.dims_ = {rows, cols};
        m.v_.resize(nnz);
        m.row_index_.resize(rows + 1);
        m.col_index_.resize(nnz);
        // usize Vecs filled in place (the library widens int32 columns on the device)
        detail::check(bsm_csr_download(h.get(), reinterpret_cast<uint64_t*>(m.row_index_.data()),
                                       reinterpret_cast<uint64_t*>(m.col_index_.data()), m.v_.data()));
        m.is_finalised_ = true;  // what finalise() leaves (sparse.rs:206-219)
        m.dev_ = std::move(h);
        return m;
    }

private:
    MatDim dims_;
    std::vector<T> v_;
    std::vector<size_t> col_index_;
    std::vector<size_t> row_index_;
    bool is_finalised_ = false;
    size_t iter_v_index_ = 0, iter_row_index_ = 0;
    mutable detail::Handle dev_;
    mutable detail::MultiCopy mdev_;
};

template <class T>
Csr<T> Csr<T>::from(const COO<T>& coo) requires detail::GpuScalar<T> {
    const auto& es = coo.entries();
    std::vector<uint64_t> r(es.size()), c(es.size());
    std::vector<T> v(es.size());
    for (size_t i = 0; i < es.size(); ++i) {
        r[i] = es[i].row;
        c[i] = es[i].col;
        v[i] = es[i].value;
    }
    bsm_csr* out = nullptr;
    if (auto e = detail::status(bsm_csr_from_coo(detail::dtype_of<T>::value, coo.dims().rows, coo.dims().cols,
                                                 es.size(), r.data(), c.data(), v.data(), &out)))
        throw Panic(std::string("COO entry out of bounds: ") + to_string(*e));
    return from_device(detail::Handle(out, detail::HandleFree{}));
}

// ----------------------------------------------------------------- lib.rs
namespace detail {
template <class T>
Dense<T> run_solver(int (*fn)(const bsm_csr*, uint64_t, uint64_t, const void* const*, void* const*),
                    const Csr<T>& m, const Dense<T>& rhs) {
    const size_t n = rhs.get_dims().rows, k = rhs.get_dims().cols;
    if (m.get_dims().rows < n) throw Panic("index out of bounds: matrix has fewer rows than the right-hand side");
    auto h = m.device();
    Dense<T> out = Dense<T>::new_default_with_dims(k, n);
    std::vector<const void*> in_cols(k);
    std::vector<void*> out_cols(k);
    for (size_t j = 0; j < k; ++j) {
        in_cols[j] = rhs.get_col(j).data();
        out_cols[j] = out.get_col_mut(j).data();
    }
    check(fn(h.get(), k, n, in_cols.data(), out_cols.data()));
    return out;
}
}  // namespace detail

/// lib.rs:28-46: solve L y = b (the diagonal is the LAST entry of each row).
template <class T>
    requires std::is_floating_point_v<T>
Dense<T> forward_substitution(Csr<T> l, Dense<T> b) {
    return detail::run_solver<T>(bsm_forward_substitution, l, b);
}

/// lib.rs:49-65: solve L* x = y (the diagonal is the FIRST entry of each row).
template <class T>
    requires std::is_floating_point_v<T>
Dense<T> backward_substitution(Csr<T> l_star, Dense<T> y) {
    return detail::run_solver<T>(bsm_backward_substitution, l_star, y);
}

/// lib.rs:11-24 (f32 in the reference; f64 is this build's addition). A
/// non-square `a` panics (`cholesky_decomp().unwrap()`, lib.rs:20).
template <class T>
    requires std::is_floating_point_v<T>
Dense<T> solve(Csr<T> a, Dense<T> b) {
    if (a.get_dims().rows != a.get_dims().cols)
        throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
    return detail::run_solver<T>(bsm_solve, a, b);
}

/// solve with the sums reassociated (bsm_solve_blocked; this build's
/// addition): within the f64 tolerance, not bit-exact; same errors/panics.
template <class T>
    requires std::is_floating_point_v<T>
Dense<T> solve_blocked(Csr<T> a, Dense<T> b) {
    if (a.get_dims().rows != a.get_dims().cols)
        throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
    return detail::run_solver<T>(bsm_solve_blocked, a, b);
}

/// solve by a nested-dissection multifrontal factor of P A P^T (bsm_solve_nd;
/// this build's addition): within the f64 tolerance, not bit-exact; the
/// ordering plan is cached on the device handle; same errors/panics.
template <class T>
    requires std::is_floating_point_v<T>
Dense<T> solve_nd(Csr<T> a, Dense<T> b) {
    if (a.get_dims().rows != a.get_dims().cols)
        throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
    return detail::run_solver<T>(bsm_solve_nd, a, b);
}

/// The system an NdFactor solves (BSM_ND_SYS_*).
enum class NdSystem : int { A = BSM_ND_SYS_A, L = BSM_ND_SYS_L, Lt = BSM_ND_SYS_LT };

/// What NdFactor::solve_refined returns: x (the iterate with the smallest
/// backward error), and per right-hand column the corrections made, that
/// backward error, whether it is at or below tol, and the tol in use.
template <class T>
struct Refined {
    Dense<T> x;
    std::vector<uint32_t> iters;
    std::vector<double> berr;
    std::vector<bool> converged;
    double tol = 0.0;
};

/// What NdFactor::solve_pcg returns: x, and per right-hand column the CG steps
/// made, the backward error of x's true residual, whether it is at or below
/// tol, whether the column broke down (S or the factor not positive definite:
/// x is that of its last completed step), and the tol in use.
template <class T>
struct Pcg {
    Dense<T> x;
    std::vector<uint32_t> iters;
    std::vector<double> berr;
    std::vector<bool> converged;
    std::vector<bool> breakdown;
    double tol = 0.0;
};

/// What NdFactor::eigsh returns: lam ascending, the unit eigenvectors as the
/// columns of `vectors`, the true residuals ||S y - lam y||2 / ||y||2, the
/// Lanczos steps, the basis columns used, the number of pairs whose residual
/// estimate is at or below tol, whether the block lost rank (the Krylov space
/// is invariant: pairs the basis could not give have lam NaN), whether a solve
/// ended above the refined solve's tol, and the tol in use.
template <class T>
struct Eig {
    std::vector<double> lam;
    Dense<T> vectors;
    std::vector<double> resid;
    uint32_t steps = 0;
    uint32_t ncv_used = 0;
    uint32_t converged = 0;
    bool exhausted = false;
    bool inexact = false;
    double tol = 0.0;
};

namespace detail {
/// (m + 2) 2^-53, m the longest row of a's lower triangle mirrored: the
/// library's default tol (the rounding bound of the f64 residual itself).
template <class T>
double refine_default_tol(const Csr<T>& a) {
    const size_t n = a.get_dims().rows;
    std::vector<uint64_t> len(n, 0);
    const auto& rp = a.row_index();
    const auto& ci = a.col_index();
    for (size_t i = 0; i < n; ++i)
        for (size_t e = rp[i]; e < rp[i + 1]; ++e) {
            if (ci[e] <= i) ++len[i];
            if (ci[e] < i) ++len[ci[e]];
        }
    uint64_t m = 0;
    for (uint64_t l : len) m = std::max(m, l);
    return (double)(m + 2) * 0x1p-53;
}
}  // namespace detail

/// The factor of solve_nd, kept (bsm_nd_factor; this build's addition): the
/// constructor analyses and factors P A P^T once (a non-square `a` panics,
/// one that is not positive definite throws DeviceError), solve() runs only
/// the forward and backward passes, l() / l_star() export the factor in
/// cholesky_decomp's conventions (new order; perm()[new] = old). The handle
/// owns its numeric storage (nbytes()) until it is destroyed; movable, not
/// copyable.
template <class T>
    requires std::is_floating_point_v<T>
class NdFactor {
public:
    explicit NdFactor(const Csr<T>& a) {
        if (a.get_dims().rows != a.get_dims().cols)
            throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
        auto h = a.device();
        bsm_nd_factor* f = nullptr;
        detail::check(bsm_nd_factor_create(h.get(), &f));
        f_.reset(f);
        detail::check(bsm_nd_factor_info(f, &n_, nullptr, nullptr, nullptr));
        src_dtype_ = detail::dtype_of<T>::value;
    }

    /// The factor in dtype T of a matrix of another float dtype
    /// (bsm_nd_factor_create_as; see cholesky_nd_as): a's values are rounded
    /// to T once, and the factor has the bits of NdFactor<T> on that matrix.
    template <class U>
        requires std::is_floating_point_v<U>
    static NdFactor from_matrix_of(const Csr<U>& a) {
        if (a.get_dims().rows != a.get_dims().cols)
            throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
        auto h = a.device();
        bsm_nd_factor* f = nullptr;
        detail::check(bsm_nd_factor_create_as(h.get(), detail::dtype_of<T>::value, &f));
        NdFactor out;
        out.f_.reset(f);
        detail::check(bsm_nd_factor_info(f, &out.n_, nullptr, nullptr, nullptr));
        out.src_dtype_ = detail::dtype_of<U>::value;
        return out;
    }

    /// The factor in dtype T of `a` with the Schur set `idx` (bsm_nd_factor_create_schur; see cholesky_nd_schur):
    /// distinct vertices, any order, which the analysis orders last as the separator tree's root. An index >= n,
    /// a repeated one or more than 16384 of them throw.
    template <class U>
        requires std::is_floating_point_v<U>
    static NdFactor with_schur(const Csr<U>& a, const std::vector<uint64_t>& idx) {
        if (a.get_dims().rows != a.get_dims().cols)
            throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
        auto h = a.device();
        bsm_nd_factor* f = nullptr;
        detail::check(bsm_nd_factor_create_schur(h.get(), detail::dtype_of<T>::value, idx.data(), idx.size(), &f));
        NdFactor out;
        out.f_.reset(f);
        detail::check(bsm_nd_factor_info(f, &out.n_, nullptr, nullptr, nullptr));
        out.src_dtype_ = detail::dtype_of<U>::value;
        return out;
    }

    /// The Schur set as given (empty: the factor was made without one): the order of schur()'s rows and columns.
    std::vector<uint64_t> schur_index() const {
        uint64_t m = 0;
        detail::check(bsm_nd_factor_schur_info(f_.get(), &m, nullptr));
        std::vector<uint64_t> idx(m);
        detail::check(bsm_nd_factor_schur_info(f_.get(), nullptr, idx.data()));
        return idx;
    }

    /// S = A_GG - A_GI A_II^-1 A_IG on the set G (bsm_nd_factor_schur): m x m, column-major, in schur_index()'s
    /// order; exactly symmetric. `a` is the matrix this is the factor of (its pattern is checked, its values are
    /// the caller's responsibility). Throws for a factor made without a set, and after update / downdate until a
    /// refactor.
    template <class U>
        requires std::is_floating_point_v<U>
    std::vector<T> schur(const Csr<U>& a) const {
        const size_t m = schur_index().size();
        std::vector<T> out(m * m);
        auto h = a.device();
        detail::check(bsm_nd_factor_schur(f_.get(), h.get(), out.data(), m ? m : 1));
        return out;
    }

    /// g = b_G - A_GI A_II^-1 b_I (bsm_nd_factor_schur_condense): m x k in schur_index()'s order.
    Dense<T> schur_condense(const Dense<T>& b) const {
        if (b.get_dims().rows != n_) throw Panic("NdFactor::schur_condense: IncorrectDimensions");
        const size_t k = b.get_dims().cols, m = schur_index().size();
        Dense<T> out = Dense<T>::new_default_with_dims(k, m);
        std::vector<const void*> bc(k);
        std::vector<void*> gc(k);
        for (size_t j = 0; j < k; ++j) {
            bc[j] = b.get_col(j).data();
            gc[j] = out.get_col_mut(j).data();
        }
        detail::check(bsm_nd_factor_schur_condense(f_.get(), bc.data(), k, gc.data()));
        return out;
    }

    /// x from b and a given x_G (bsm_nd_factor_schur_expand; xg: m x k in schur_index()'s order). Stateless: it
    /// repeats schur_condense's forward pass. With xg the rows schur_index() of solve(b) it returns solve(b) bit
    /// for bit.
    Dense<T> schur_expand(const Dense<T>& b, const Dense<T>& xg) const {
        const size_t k = b.get_dims().cols;
        if (b.get_dims().rows != n_ || xg.get_dims().cols != k || xg.get_dims().rows != schur_index().size())
            throw Panic("NdFactor::schur_expand: IncorrectDimensions");
        Dense<T> out = Dense<T>::new_default_with_dims(k, n_);
        std::vector<const void*> bc(k), gc(k);
        std::vector<void*> xc(k);
        for (size_t j = 0; j < k; ++j) {
            bc[j] = b.get_col(j).data();
            gc[j] = xg.get_col(j).data();
            xc[j] = out.get_col_mut(j).data();
        }
        detail::check(bsm_nd_factor_schur_expand(f_.get(), bc.data(), k, gc.data(), xc.data()));
        return out;
    }

    size_t rows() const { return n_; }

    /// New values on the same pattern (bsm_nd_factor_refactor): afterwards the
    /// factor has the bits of NdFactor(a) (of cholesky_nd_as<T>(a) for a
    /// matrix of the other float dtype). A dtype other than the factored
    /// matrix's, another shape or pattern throws and leaves the factor untouched. Values
    /// that are not positive definite throw DeviceError and leave the handle
    /// without a factor until a later refactor succeeds.
    template <class U>
        requires std::is_floating_point_v<U>
    void refactor(const Csr<U>& a) {
        if (a.get_dims().rows != a.get_dims().cols)
            throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
        auto h = a.device();
        detail::check(bsm_nd_factor_refactor(f_.get(), h.get()));
    }

    /// New values at the named places (rows[e], cols[e]) of the factored
    /// pattern alone (bsm_nd_factor_refactor_partial): only the fronts on the
    /// paths from those entries to the roots are factored again, and the
    /// factor has the bits refactor(a) gives. a equals the factored matrix in
    /// every other stored entry with col <= row; no update / downdate has run
    /// since the last factorisation (else DeviceError: refactor first). A pair
    /// that is not stored, an index >= n, another pattern or dtype throw and
    /// leave the factor untouched. Returns {fronts factored again, fronts in
    /// the plan, changed entries}.
    template <class U>
        requires std::is_floating_point_v<U>
    std::array<uint64_t, 3> refactor_partial(const Csr<U>& a, const std::vector<uint64_t>& rows,
                                             const std::vector<uint64_t>& cols) {
        if (a.get_dims().rows != a.get_dims().cols)
            throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
        if (rows.size() != cols.size())
            throw std::invalid_argument("NdFactor::refactor_partial: rows and cols differ in length");
        auto h = a.device();
        std::array<uint64_t, 3> info{0, 0, 0};
        detail::check(bsm_nd_factor_refactor_partial(f_.get(), h.get(), rows.size(), rows.data(), cols.data(),
                                                     info.data()));
        return info;
    }

    /// The same with the places found on the device (bsm_nd_factor_refactor_since):
    /// the stored entries with col <= row whose bits differ between a_old (the
    /// matrix this is the factor of) and a_new.
    template <class U>
        requires std::is_floating_point_v<U>
    std::array<uint64_t, 3> refactor_since(const Csr<U>& a_old, const Csr<U>& a_new) {
        if (a_new.get_dims().rows != a_new.get_dims().cols)
            throw Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix");
        auto ho = a_old.device();
        auto hn = a_new.device();
        std::array<uint64_t, 3> info{0, 0, 0};
        detail::check(bsm_nd_factor_refactor_since(f_.get(), ho.get(), hn.get(), info.data()));
        return info;
    }

    /// The factor of P (S + W W^T) P^T in place (bsm_nd_factor_updown), S the
    /// matrix this was the factor of, w of shape n x k, 1 <= k <= 16, of the
    /// FACTORED MATRIX's dtype (another one throws std::invalid_argument,
    /// another row count Panic). Only the fronts on the paths from w's columns
    /// to the root are rewritten. A column is inside when, with its entry
    /// that comes first in the new order (perm()) in tree node N, every other
    /// entry is an own column or a front row of N: always so for alpha e_i and
    /// for a vertex with any of its neighbours in S's graph that come later in
    /// the new order (an edge of a stored (i, j)). A column outside, a row
    /// >= n or k > 16 throws DeviceError before anything is written.
    template <class U>
        requires std::is_floating_point_v<U>
    void update(const Csr<U>& w) { updown(w, +1, "NdFactor::update"); }

    /// The factor of P (S - W W^T) P^T in place: update's arguments and
    /// errors. A w that leaves the matrix not positive definite throws
    /// DeviceError; the factor keeps its bits and stays valid.
    template <class U>
        requires std::is_floating_point_v<U>
    void downdate(const Csr<U>& w) { updown(w, -1, "NdFactor::downdate"); }

    /// x = A^-1 b for a SPARSE b (n x k, of the factor's dtype), x wanted at
    /// `rows` only (bsm_nd_factor_solve_sparse): result row e is x[rows[e]]
    /// (A's order, unsorted and repeated as the caller likes); rows == nullptr:
    /// every row. Only the fronts on the paths from b's entries and from the
    /// requested rows' fronts to the root are visited, with the dense solve's
    /// operations in its order: every value equals solve()'s on the densified
    /// b (a zero may differ in sign). info: the C call's four counts, or null.
    /// Another row count: Panic; a row >= n throws as the C call reports it.
    Dense<T> solve_sparse(const Csr<T>& b, const std::vector<uint64_t>* rows = nullptr,
                          std::array<uint32_t, 4>* info = nullptr) const {
        if (b.get_dims().rows != n_) throw Panic("NdFactor::solve_sparse: IncorrectDimensions");
        // column-compressed: a counting sort by column keeps the rows ascending within each
        const size_t k = b.get_dims().cols, nnz = b.v().size();
        std::vector<uint64_t> cp(k + 1, 0), br(nnz);
        std::vector<T> vals(nnz);
        for (size_t c : b.col_index()) ++cp[c + 1];
        for (size_t c = 0; c < k; ++c) cp[c + 1] += cp[c];
        std::vector<uint64_t> at(cp.begin(), cp.end() - 1);
        const auto& rp = b.row_index();
        for (size_t r = 0; r + 1 < rp.size(); ++r)
            for (size_t e = rp[r]; e < rp[r + 1]; ++e) {
                const uint64_t o = at[b.col_index()[e]]++;
                br[o] = r;
                vals[o] = b.v()[e];
            }
        return solve_sparse_cc(k, cp, br, vals, rows, info);
    }

    /// A^-1[rows, cols] for ANY rows and columns (A's order), row-major
    /// rows.size() x cols.size(): solve_sparse of the unit columns e_cols at
    /// `rows`. Where inv_entries refuses a pair off the pattern of L + L^T,
    /// this answers.
    std::vector<T> inv_block(const std::vector<uint64_t>& rows, const std::vector<uint64_t>& cols) const {
        const size_t k = cols.size(), nq = rows.size();
        std::vector<uint64_t> cp(k + 1);
        for (size_t c = 0; c <= k; ++c) cp[c] = c;
        const Dense<T> x = solve_sparse_cc(k, cp, cols, std::vector<T>(k, T(1)), &rows, nullptr);
        std::vector<T> out(nq * k);
        for (size_t j = 0; j < k; ++j)
            for (size_t i = 0; i < nq; ++i) out[i * k + j] = x.get_col(j)[i];
        return out;
    }

    /// log det A = 2 sum log L_ii, summed in f64 in a fixed order.
    double logdet() const {
        double v = 0.0;
        detail::check(bsm_nd_factor_logdet(f_.get(), &v));
        return v;
    }

    /// x = A^-1 b: column j has the bits of solve_nd's column j (one column:
    /// of solve_nd with BSM_ND_FOLD=0). NdSystem::L: L y = b; NdSystem::Lt:
    /// L^T x = y, both in the NEW order (perm(), l()): nothing is permuted.
    Dense<T> solve(const Dense<T>& b, NdSystem system = NdSystem::A) const {
        const size_t n = b.get_dims().rows, k = b.get_dims().cols;
        Dense<T> out = Dense<T>::new_default_with_dims(k, n);
        std::vector<const void*> in_cols(k);
        std::vector<void*> out_cols(k);
        for (size_t j = 0; j < k; ++j) {
            in_cols[j] = b.get_col(j).data();
            out_cols[j] = out.get_col_mut(j).data();
        }
        detail::check(bsm_nd_factor_solve_system(f_.get(), static_cast<int>(system), k, n, in_cols.data(),
                                                 out_cols.data()));
        return out;
    }

    /// Iterative refinement on this factor (bsm_nd_factor_solve_refined):
    /// x_0 = M^-1 b, then up to max_iter corrections from f64 residuals of
    /// S x = b, S being a's lower triangle mirrored; every column on its own.
    /// `a` (f32 or f64, the factored matrix or one near it) and b share a
    /// dtype, which need not be the factor's. tol == 0: (m + 2) 2^-53, m the
    /// longest row of S. a or b of another shape: Panic (IncorrectDimensions).
    template <class U>
        requires std::is_floating_point_v<U>
    Refined<U> solve_refined(const Csr<U>& a, const Dense<U>& b, unsigned max_iter = 5, double tol = 0) const {
        const size_t n = b.get_dims().rows, k = b.get_dims().cols;
        if (!(tol >= 0)) throw std::invalid_argument("NdFactor::solve_refined: tol must be >= 0 (0 = the default)");
        if (a.get_dims().rows != n_ || a.get_dims().cols != n_ || n != n_)
            throw Panic("NdFactor::solve_refined: IncorrectDimensions");
        Refined<U> out{Dense<U>::new_default_with_dims(k, n), std::vector<uint32_t>(k), std::vector<double>(k),
                       std::vector<bool>(k), tol > 0 ? tol : detail::refine_default_tol(a)};
        std::vector<const void*> in_cols(k);
        std::vector<void*> out_cols(k);
        for (size_t j = 0; j < k; ++j) {
            in_cols[j] = b.get_col(j).data();
            out_cols[j] = out.x.get_col_mut(j).data();
        }
        auto h = a.device();
        detail::check(bsm_nd_factor_solve_refined(f_.get(), h.get(), k, n, in_cols.data(), out_cols.data(), max_iter,
                                                  out.tol, out.iters.data(), out.berr.data()));
        for (size_t j = 0; j < k; ++j) out.converged[j] = out.berr[j] <= out.tol;
        return out;
    }

    /// Preconditioned conjugate gradients on this factor
    /// (bsm_nd_factor_solve_pcg): S x = b with the factor's solve as
    /// preconditioner, every column its own CG, everything but that solve in
    /// f64. Arguments, tol and the first iterate are solve_refined's; it
    /// converges for any positive definite `a` (a stale factor, 3 A, a
    /// low-rank change), in at most max_iter steps.
    template <class U>
        requires std::is_floating_point_v<U>
    Pcg<U> solve_pcg(const Csr<U>& a, const Dense<U>& b, unsigned max_iter = 50, double tol = 0) const {
        const size_t n = b.get_dims().rows, k = b.get_dims().cols;
        if (!(tol >= 0)) throw std::invalid_argument("NdFactor::solve_pcg: tol must be >= 0 (0 = the default)");
        if (a.get_dims().rows != n_ || a.get_dims().cols != n_ || n != n_)
            throw Panic("NdFactor::solve_pcg: IncorrectDimensions");
        Pcg<U> out{Dense<U>::new_default_with_dims(k, n), std::vector<uint32_t>(k), std::vector<double>(k),
                   std::vector<bool>(k), std::vector<bool>(k), tol > 0 ? tol : detail::refine_default_tol(a)};
        std::vector<const void*> in_cols(k);
        std::vector<void*> out_cols(k);
        for (size_t j = 0; j < k; ++j) {
            in_cols[j] = b.get_col(j).data();
            out_cols[j] = out.x.get_col_mut(j).data();
        }
        std::vector<uint32_t> flags(k);
        auto h = a.device();
        detail::check(bsm_nd_factor_solve_pcg(f_.get(), h.get(), k, n, in_cols.data(), out_cols.data(), max_iter,
                                              out.tol, out.iters.data(), out.berr.data(), flags.data()));
        for (size_t j = 0; j < k; ++j) {
            out.converged[j] = out.berr[j] <= out.tol;
            out.breakdown[j] = (flags[j] & 1u) != 0;
        }
        return out;
    }

    /// The nev smallest eigenvalues of S (a's lower triangle mirrored) and
    /// their eigenvectors by block shift-invert Lanczos on this factor
    /// (bsm_nd_factor_eigsh): A^-1 by the refined solve, `block` columns at a
    /// time, full reorthogonalisation, at most ncv basis columns (0: min(n,
    /// 128); rounded down to a multiple of block). tol == 0: 2^-26 for f64,
    /// 2^-12 for f32. v0: an n x block start block, or null for the one made
    /// from `seed`. Bad arguments throw as the C call reports them.
    template <class U>
        requires std::is_floating_point_v<U>
    Eig<U> eigsh(const Csr<U>& a, size_t nev, size_t block = 4, size_t ncv = 0, double tol = 0,
                 const Dense<U>* v0 = nullptr, uint64_t seed = 0) const {
        if (!(tol >= 0)) throw std::invalid_argument("NdFactor::eigsh: tol must be >= 0 (0 = the default)");
        if (a.get_dims().rows != n_ || a.get_dims().cols != n_ ||
            (v0 && (v0->get_dims().rows != n_ || v0->get_dims().cols != block)))
            throw Panic("NdFactor::eigsh: IncorrectDimensions");
        if (n_ == 0) nev = 0;
        Eig<U> out{std::vector<double>(nev), Dense<U>::new_default_with_dims(nev, n_), std::vector<double>(nev)};
        out.tol = tol > 0 ? tol : (sizeof(U) == 8 ? 0x1p-26 : 0x1p-12);
        if (n_ == 0) return out;
        std::vector<const void*> in_cols(v0 ? block : 0);
        for (size_t j = 0; j < in_cols.size(); ++j) in_cols[j] = v0->get_col(j).data();
        std::vector<void*> out_cols(nev);
        for (size_t j = 0; j < nev; ++j) out_cols[j] = out.vectors.get_col_mut(j).data();
        uint32_t info[4] = {0, 0, 0, 0};
        double none = 0.0;  // nev == 0 is refused by the library, not by a null pointer here
        auto h = a.device();
        detail::check(bsm_nd_factor_eigsh(f_.get(), h.get(), nev, block, ncv, out.tol, seed,
                                          v0 ? in_cols.data() : nullptr, nev ? out.lam.data() : &none,
                                          out_cols.data(), nev ? out.resid.data() : &none, info));
        out.steps = info[0];
        out.ncv_used = info[1];
        out.converged = info[2];
        out.exhausted = (info[3] & 1u) != 0;
        out.inexact = (info[3] & 2u) != 0;
        return out;
    }

    /// eigsh for the generalised problem S y = lam S_M y (bsm_nd_factor_eigsh_gen):
    /// m is the mass matrix, n x n of a's type with any pattern, S_M its lower
    /// triangle mirrored, which must be positive definite (else the call throws
    /// "m is not positive definite"). The same loop in the S_M inner product:
    /// the vectors have y^T S_M y = 1 and resid is ||S y - lam S_M y||2 / ||y||2.
    /// The other arguments and the result are eigsh's.
    template <class U>
        requires std::is_floating_point_v<U>
    Eig<U> eigsh_gen(const Csr<U>& a, const Csr<U>& m, size_t nev, size_t block = 4, size_t ncv = 0, double tol = 0,
                     uint64_t seed = 0, const Dense<U>* v0 = nullptr) const {
        if (!(tol >= 0)) throw std::invalid_argument("NdFactor::eigsh_gen: tol must be >= 0 (0 = the default)");
        if (a.get_dims().rows != n_ || a.get_dims().cols != n_ || m.get_dims().rows != n_ ||
            m.get_dims().cols != n_ || (v0 && (v0->get_dims().rows != n_ || v0->get_dims().cols != block)))
            throw Panic("NdFactor::eigsh_gen: IncorrectDimensions");
        if (n_ == 0) nev = 0;
        Eig<U> out{std::vector<double>(nev), Dense<U>::new_default_with_dims(nev, n_), std::vector<double>(nev)};
        out.tol = tol > 0 ? tol : (sizeof(U) == 8 ? 0x1p-26 : 0x1p-12);
        if (n_ == 0) return out;
        std::vector<const void*> in_cols(v0 ? block : 0);
        for (size_t j = 0; j < in_cols.size(); ++j) in_cols[j] = v0->get_col(j).data();
        std::vector<void*> out_cols(nev);
        for (size_t j = 0; j < nev; ++j) out_cols[j] = out.vectors.get_col_mut(j).data();
        uint32_t info[4] = {0, 0, 0, 0};
        double none = 0.0;  // nev == 0 is refused by the library, not by a null pointer here
        auto h = a.device();
        auto hm = m.device();
        detail::check(bsm_nd_factor_eigsh_gen(f_.get(), h.get(), hm.get(), nev, block, ncv, out.tol, seed,
                                              v0 ? in_cols.data() : nullptr, nev ? out.lam.data() : &none,
                                              out_cols.data(), nev ? out.resid.data() : &none, info));
        out.steps = info[0];
        out.ncv_used = info[1];
        out.converged = info[2];
        out.exhausted = (info[3] & 1u) != 0;
        out.inexact = (info[3] & 2u) != 0;
        return out;
    }

    /// diag(A^-1) in A's order (bsm_nd_factor_selinv): the selected inverse by
    /// the Takahashi recursion over the fronts; the same bits on every call.
    std::vector<T> inv_diag() const {
        std::vector<T> d(n_);
        if (n_ > 0) detail::check(bsm_nd_factor_selinv(f_.get(), d.data(), 0, nullptr, nullptr, nullptr));
        return d;
    }

    /// (A^-1)[rows[e]][cols[e]] for pairs on the pattern of L + L^T (A's order,
    /// either triangle). An index >= n or a pair outside the pattern throws.
    std::vector<T> inv_entries(const std::vector<uint64_t>& rows, const std::vector<uint64_t>& cols) const {
        if (rows.size() != cols.size()) throw std::invalid_argument("NdFactor::inv_entries: rows and cols differ in length");
        std::vector<T> v(rows.size());
        if (!rows.empty())
            detail::check(bsm_nd_factor_selinv(f_.get(), nullptr, rows.size(), rows.data(), cols.data(), v.data()));
        return v;
    }

    /// perm[new] = old.
    std::vector<int64_t> perm() const {
        std::vector<int64_t> p(n_);
        detail::check(bsm_nd_factor_perm(f_.get(), p.data()));
        return p;
    }

    /// L: rows ascending, the diagonal LAST (forward_substitution's operand).
    Csr<T> l() const {
        bsm_csr* out = nullptr;
        detail::check(bsm_nd_factor_export(f_.get(), &out, nullptr));
        return Csr<T>::from_device(detail::Handle(out, detail::HandleFree{}));
    }

    /// L^T: the diagonal FIRST (backward_substitution's operand).
    Csr<T> l_star() const {
        bsm_csr* out = nullptr;
        detail::check(bsm_nd_factor_export(f_.get(), nullptr, &out));
        return Csr<T>::from_device(detail::Handle(out, detail::HandleFree{}));
    }

    /// Device bytes the handle owns.
    uint64_t nbytes() const {
        uint64_t b = 0;
        detail::check(bsm_nd_factor_info(f_.get(), nullptr, nullptr, &b, nullptr));
        return b;
    }

private:
    NdFactor() = default;
    // b column-compressed; an empty `rows` is passed as a non-null pointer (null means every row)
    Dense<T> solve_sparse_cc(size_t k, const std::vector<uint64_t>& cp, const std::vector<uint64_t>& br,
                             const std::vector<T>& vals, const std::vector<uint64_t>* rows,
                             std::array<uint32_t, 4>* info) const {
        const size_t nout = rows ? rows->size() : n_;
        Dense<T> out = Dense<T>::new_default_with_dims(k, nout);
        std::vector<void*> out_cols(k);
        for (size_t j = 0; j < k; ++j) out_cols[j] = out.get_col_mut(j).data();
        const uint64_t none = 0;
        uint32_t inf[4] = {0, 0, 0, 0};
        detail::check(bsm_nd_factor_solve_sparse(f_.get(), k, cp.data(), br.data(), vals.data(), rows ? rows->size() : 0,
                                                 rows ? (rows->empty() ? &none : rows->data()) : nullptr,
                                                 out_cols.data(), inf));
        if (info) *info = {inf[0], inf[1], inf[2], inf[3]};
        return out;
    }
    template <class U>
    void updown(const Csr<U>& w, int sign, const char* what) {
        if (w.get_dims().rows != n_) throw Panic(std::string(what) + ": IncorrectDimensions");
        if (detail::dtype_of<U>::value != src_dtype_)
            throw std::invalid_argument(std::string(what) + ": w must have the factored matrix's dtype");
        // column-compressed: a counting sort by column keeps the rows ascending within each
        const size_t k = w.get_dims().cols, nnz = w.v().size();
        std::vector<uint64_t> cp(k + 1, 0), rows(nnz);
        std::vector<U> vals(nnz);
        for (size_t c : w.col_index()) ++cp[c + 1];
        for (size_t c = 0; c < k; ++c) cp[c + 1] += cp[c];
        std::vector<uint64_t> at(cp.begin(), cp.end() - 1);
        const auto& rp = w.row_index();
        for (size_t r = 0; r + 1 < rp.size(); ++r)
            for (size_t e = rp[r]; e < rp[r + 1]; ++e) {
                const uint64_t o = at[w.col_index()[e]]++;
                rows[o] = r;
                vals[o] = w.v()[e];
            }
        detail::check(bsm_nd_factor_updown(f_.get(), sign, k, cp.data(), rows.data(), vals.data()));
    }
    struct Free {
        void operator()(bsm_nd_factor* p) const { bsm_nd_factor_free(p); }
    };
    std::unique_ptr<bsm_nd_factor, Free> f_;
    uint64_t n_ = 0;
    int src_dtype_ = detail::dtype_of<T>::value;  // the factored matrix's dtype (update / downdate take W in it)
};

/// The nd factor of `a` computed and kept in dtype F (this build's addition):
/// an f32 factor of an f64 matrix has half the bytes; NdFactor::solve_refined
/// brings its solves back to f64 accuracy.
template <class F, class T>
    requires std::is_floating_point_v<F> && std::is_floating_point_v<T>
NdFactor<F> cholesky_nd_as(const Csr<T>& a) {
    return NdFactor<F>::from_matrix_of(a);
}

/// The nd factor of `a` in dtype F with the Schur set `idx` (this build's addition): NdFactor::schur,
/// schur_condense and schur_expand then give the Schur complement on those vertices, its right-hand side and the
/// expansion of its solution; every other method works as on any factor, and refactor keeps the set.
template <class F, class T>
    requires std::is_floating_point_v<F> && std::is_floating_point_v<T>
NdFactor<F> cholesky_nd_schur(const Csr<T>& a, const std::vector<uint64_t>& idx) {
    return NdFactor<F>::with_schur(a, idx);
}

}  // namespace bsm

#endif  // BSM_HPP
