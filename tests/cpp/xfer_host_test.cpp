// The host helpers of the transfer pipelines (csrc/xfer_host.hpp: par_memcpy
// and Prefault) on the CPU, built by tests/test_xfer_host.py once with
// -fsanitize=thread and once with -fsanitize=address,undefined.
//
// par_memcpy: every thread count 1..16 at the sizes around its 4 MiB threshold
// and at n = t * 4096 * m + r (floor(n / t) a multiple of the page, r bytes
// over: the sizes at which a floor-rounded part leaves the tail uncopied),
// source and destination at odd offsets, 0xA5 guards on both sides, the result
// compared with memcpy's.
// Prefault: an unaligned range whose length is no multiple of the chunk; every
// wait(i) returns; only one byte per 4 KiB step of each chunk is written (a
// zero) and nothing outside [p, p + bytes); finish() before the chunks are all
// taken; no threads; the no-op below 8 MiB.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "xfer_host.hpp"

namespace {

int failed = 0, checks = 0;

void expect(bool ok, const char* what, long a = 0, long b = 0) {
    ++checks;
    if (ok) return;
    ++failed;
    if (failed <= 20) std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
}

constexpr size_t GUARD = 64;
constexpr unsigned char FILL = 0xA5;

uint64_t counter(bsm::XferCounter c) { return bsm::g_xfer_counters[c].load(std::memory_order_relaxed); }

// first index at which a and b differ, or -1
long first_diff(const unsigned char* a, const unsigned char* b, size_t n) {
    if (std::memcmp(a, b, n) == 0) return -1;
    for (size_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return (long)i;
    return -1;
}

bool all_fill(const unsigned char* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (p[i] != FILL) return false;
    return true;
}

void copy_case(const std::vector<unsigned char>& pattern, size_t n, int t, size_t src_off, size_t dst_off) {
    std::vector<unsigned char> got(dst_off + GUARD + n + GUARD, FILL), want(n);
    const unsigned char* src = pattern.data() + src_off;
    std::memcpy(want.data(), src, n);
    unsigned char* dst = got.data() + dst_off + GUARD;
    const uint64_t threaded0 = counter(bsm::XFER_PAR_MEMCPY_THREADED);
    bsm::par_memcpy(dst, src, n, t);
    expect(first_diff(dst, want.data(), n) < 0, "par_memcpy differs from memcpy at (n, threads); first index follows",
           (long)n, t);
    if (first_diff(dst, want.data(), n) >= 0 && failed <= 20)
        std::printf("     first mismatching byte %ld of %zu\n", first_diff(dst, want.data(), n), n);
    expect(all_fill(got.data(), dst_off + GUARD), "guard before the destination written", (long)n, t);
    expect(all_fill(dst + n, GUARD), "guard after the destination written", (long)n, t);
    const bool threaded = counter(bsm::XFER_PAR_MEMCPY_THREADED) == threaded0 + 1;
    expect(threaded == (t > 1 && n >= bsm::PAR_MEMCPY_MIN), "threaded-copy counter", (long)n, t);
}

void test_par_memcpy() {
    const size_t M4 = 4ull << 20, MAXN = 16 * 4096 * 70 + 4096;
    std::vector<unsigned char> pattern(MAXN + 16);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto& b : pattern) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = (unsigned char)(x >> 56);
        if (b == FILL) b = 0x5A;  // an uncopied byte always shows
    }
    for (int t = 1; t <= 16; ++t) {
        for (size_t n : {M4 - 4, M4, M4 + 4}) copy_case(pattern, n, t, 1, 3);
        const size_t m0 = (1024 + t - 1) / t;  // t * 4096 * m0 >= 4 MiB
        for (size_t m : {m0, m0 + 5})
            for (size_t r : {0, 4, 8, 12}) copy_case(pattern, (size_t)t * 4096 * m + r, t, 5, 1);
    }
    copy_case(pattern, 1, 8, 1, 1);
    copy_case(pattern, 4099, 16, 1, 1);  // small: one thread
}

struct Region {
    std::vector<unsigned char> mem;
    unsigned char* p;
    size_t bytes;
    Region(size_t off, size_t n) : mem(off + n + 8192, FILL), p(mem.data() + off), bytes(n) {}
    bool outside_untouched() const {
        return all_fill(mem.data(), (size_t)(p - mem.data())) &&
               all_fill(p + bytes, mem.size() - (size_t)(p - mem.data()) - bytes);
    }
};

// chunk i after Prefault: a zero at every 4096th byte from the chunk's start
// (all of them when `whole`), the fill everywhere else
bool chunk_ok(const Region& r, size_t chunk, size_t i, bool whole, bool* any_zero) {
    const size_t off = i * chunk, len = std::min(chunk, r.bytes - off);
    size_t zeros = 0;
    for (size_t o = 0; o < len; ++o) {
        const unsigned char b = r.p[off + o];
        if (o % 4096 == 0 && b == 0) ++zeros;
        else if (b != FILL) return false;
    }
    *any_zero = zeros > 0;
    return whole ? zeros == (len + 4095) / 4096 : (zeros == 0 || zeros == (len + 4095) / 4096);
}

void test_prefault() {
    const size_t M8 = 8ull << 20;
    {  // unaligned start, a tail chunk, several threads: wait(i) then read chunk i
        const size_t chunk = 1ull << 20;
        Region r(4096 + 7, M8 + 12345);
        const uint64_t c0 = counter(bsm::XFER_PREFAULT_CHUNKS);
        bsm::Prefault pf(reinterpret_cast<char*>(r.p), r.bytes, chunk, 8);
        const size_t n = (r.bytes + chunk - 1) / chunk;
        expect(pf.chunks() == n, "Prefault chunk count", (long)pf.chunks(), (long)n);
        for (size_t i = 0; i < n + 2; ++i) {
            pf.wait(i);
            bool z = false;
            if (i < n) expect(chunk_ok(r, chunk, i, true, &z), "chunk not faulted in after wait(i)", (long)i);
        }
        pf.finish();
        expect(r.outside_untouched(), "Prefault wrote outside [p, p + bytes)");
        expect(counter(bsm::XFER_PREFAULT_CHUNKS) == c0 + n, "prefault counter", (long)(counter(bsm::XFER_PREFAULT_CHUNKS) - c0));
    }
    {  // 32 threads for 9 chunks: most threads find nothing to take
        const size_t chunk = 1ull << 20;
        Region r(1, M8 + 1);
        bsm::Prefault pf(reinterpret_cast<char*>(r.p), r.bytes, chunk, 32);
        for (size_t i = 0; i < 9; ++i) pf.wait(i);
        pf.finish();
        bool z = false;
        for (size_t i = 0; i < 9; ++i) expect(chunk_ok(r, chunk, i, true, &z), "chunk not faulted in (32 threads)", (long)i);
        expect(r.outside_untouched(), "Prefault wrote outside [p, p + bytes) (32 threads)");
    }
    {  // finish() while one thread has 129 chunks to go: every wait(i) still returns
        const size_t chunk = 1ull << 16;
        Region r(4096 + 13, M8 + 100);
        const size_t n = (r.bytes + chunk - 1) / chunk;
        bsm::Prefault pf(reinterpret_cast<char*>(r.p), r.bytes, chunk, 1);
        pf.finish();
        for (size_t i = 0; i < n; ++i) pf.wait(i);
        bool z = false;
        for (size_t i = 0; i < n; ++i) expect(chunk_ok(r, chunk, i, false, &z), "half-written chunk after finish()", (long)i);
        expect(r.outside_untouched(), "Prefault wrote outside [p, p + bytes) (early finish)");
    }
    {  // no threads: nothing happens, wait returns
        Region r(5, M8 + 4096);
        const uint64_t c0 = counter(bsm::XFER_PREFAULT_CHUNKS);
        bsm::Prefault pf(reinterpret_cast<char*>(r.p), r.bytes, 1ull << 20, 0);
        expect(pf.chunks() == 0, "threads = 0 is a no-op");
        pf.wait(0);
        pf.wait(8);
        pf.finish();
        expect(all_fill(r.mem.data(), r.mem.size()), "threads = 0 wrote something");
        expect(counter(bsm::XFER_PREFAULT_CHUNKS) == c0, "threads = 0 counted chunks");
    }
    {  // below 8 MiB: nothing happens
        Region r(9, M8 - 1);
        bsm::Prefault pf(reinterpret_cast<char*>(r.p), r.bytes, 1ull << 20, 8);
        expect(pf.chunks() == 0, "below 8 MiB is a no-op");
        pf.wait(0);
        pf.finish();
        expect(all_fill(r.mem.data(), r.mem.size()), "below 8 MiB wrote something");
    }
}

}  // namespace

int main() {
    test_par_memcpy();
    test_prefault();
    std::printf("%d checks, %d failed\n", checks, failed);
    return failed ? 1 : 0;
}
