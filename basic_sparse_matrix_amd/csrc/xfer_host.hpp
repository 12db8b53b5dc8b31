// xfer_host.hpp -- the host-only helpers of the transfer pipelines
// (transfer.hip): the threaded memcpy, the page prefaulter and the route
// counters. No HIP in here, so tests/cpp/xfer_host_test.cpp builds it with the
// host sanitizers and runs it on the CPU.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include <sys/mman.h>

namespace bsm {

// Which route a host transfer took (bsm_xfer_counters, include/bsm.h):
// process-wide, relaxed, bumped once per chunk or call.
enum XferCounter {
    XFER_H2D_DIRECT_CHUNKS = 0,
    XFER_H2D_STAGED_CHUNKS,
    XFER_D2H_DIRECT_CHUNKS,
    XFER_D2H_STAGED_CHUNKS,
    XFER_PREFAULT_CHUNKS,
    XFER_PAR_MEMCPY_THREADED,
    XFER_D2H_CSR_DIRECT_CALLS,
    XFER_D2H_SMALL_PINNED_CALLS,
    XFER_COUNTERS
};
inline std::atomic<uint64_t> g_xfer_counters[XFER_COUNTERS];
inline void xfer_count(XferCounter c) { g_xfer_counters[c].fetch_add(1, std::memory_order_relaxed); }

constexpr size_t PAR_MEMCPY_MIN = 4ull << 20;  // below this one thread copies
constexpr size_t PREFAULT_MIN = 8ull << 20;    // below this the DMA takes its own faults

// memcpy split over up to `threads` (1..16) threads from PAR_MEMCPY_MIN on (one
// host thread copies ~10 GB/s, PCIe moves ~50 GB/s). Each thread takes one
// page-rounded part; the parts cover [0, n).
inline void par_memcpy(void* dst, const void* src, size_t n, int threads) {
    const int t = n >= PAR_MEMCPY_MIN ? std::clamp(threads, 1, 16) : 1;
    if (t == 1) {
        std::memcpy(dst, src, n);
        return;
    }
    // ceil(n / t) rounded up to 4 KiB: t * part >= n (the floor would leave
    // the last n % t bytes uncopied whenever n / t is a multiple of 4096)
    const size_t part = ((n + t - 1) / t + 4095) & ~size_t(4095);
    std::thread th[16];
    int used = 0;
    for (int i = 1; i < t; ++i) {
        const size_t off = part * i;
        if (off >= n) break;
        th[used++] = std::thread([=] { std::memcpy(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off,
                                                   std::min(part, n - off)); });
    }
    std::memcpy(dst, src, std::min(part, n));
    for (int i = 0; i < used; ++i) th[i].join();
    if (used) xfer_count(XFER_PAR_MEMCPY_THREADED);
}

// Fault in [p, p + bytes) chunk by chunk from `threads` (0..32) threads: a
// write per 4 KiB page; wait(i) returns once chunk i is in.
class Prefault {
public:
    Prefault(char* p, size_t bytes, size_t chunk, int threads) : p_(p), bytes_(bytes), chunk_(chunk) {
        threads = std::clamp(threads, 0, 32);
        n_ = (bytes + chunk - 1) / chunk;
        if (threads == 0 || bytes < PREFAULT_MIN) {
            n_ = 0;  // small: the DMA takes its own faults
            return;
        }
        // transparent huge pages for the 2 MiB-aligned interior (advice only;
        // the box runs THP in madvise mode): 520 MB faults in 3.8 ms on 8
        // threads with it, 30-40 ms without (profiles/r03_e_first_touch.log)
        const uintptr_t a0 = ((uintptr_t)p + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
        const uintptr_t a1 = ((uintptr_t)p + bytes) & ~(uintptr_t)((2u << 20) - 1);
        if (a1 > a0) (void)madvise((void*)a0, a1 - a0, MADV_HUGEPAGE);
        ready_.reset(new std::atomic<int>[n_]);
        for (size_t i = 0; i < n_; ++i) ready_[i].store(0, std::memory_order_relaxed);
        for (int t = 0; t < threads; ++t)
            th_.emplace_back([this] {
                for (;;) {
                    const size_t i = next_.fetch_add(1, std::memory_order_relaxed);
                    if (i >= n_ || stop_.load(std::memory_order_relaxed)) return;
                    char* q = p_ + i * chunk_;
                    const size_t len = std::min(chunk_, bytes_ - i * chunk_);
                    for (size_t o = 0; o < len; o += 4096) reinterpret_cast<volatile char*>(q)[o] = 0;
                    ready_[i].store(1, std::memory_order_release);
                    xfer_count(XFER_PREFAULT_CHUNKS);
                }
            });
    }
    size_t chunks() const { return n_; }  // 0 when it does nothing
    void wait(size_t i) {
        if (i >= n_) return;
        // after finish() an untaken chunk stays out: its copy takes the faults
        while (!ready_[i].load(std::memory_order_acquire) && !th_.empty()) std::this_thread::yield();
    }
    void finish() {
        stop_.store(true, std::memory_order_relaxed);
        for (auto& t : th_) t.join();
        th_.clear();
    }
    ~Prefault() { finish(); }

private:
    char* p_;
    size_t bytes_, chunk_, n_ = 0;
    std::unique_ptr<std::atomic<int>[]> ready_;
    std::atomic<size_t> next_{0};
    std::atomic<bool> stop_{false};
    std::vector<std::thread> th_;
};

}  // namespace bsm
