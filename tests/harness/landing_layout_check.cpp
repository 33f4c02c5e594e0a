// Stand-alone check of ompi_amd/csrc/coll_landing.h (tests/test_landing_layout_cpu.py
// builds it with -fsanitize=address,undefined and runs it).  The formulas
// below are the ones the collectives typed out by hand before the header
// existed, written here a second time; the header must give the same bytes,
// results must end inside `need`, and the input slots must end before the
// result area.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../ompi_amd/csrc/coll_landing.h"

using namespace ompi_amd;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failures <= 20) {                        \
                fprintf(stderr, "FAIL %s: ", #cond);       \
                fprintf(stderr, __VA_ARGS__);              \
                fprintf(stderr, "\n");                     \
            }                                              \
        }                                                  \
    } while (0)

static size_t R(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr size_t kCap = (2ull << 30) - (4u << 20);
constexpr size_t kStepUsable = (32u << 20) - 64;  // a landing buffer's first growth step

static size_t early_of(size_t count, size_t n) {  // blockcount()
    size_t early = count / n;
    if (count % n) early += 1;
    return early;
}

// the expressions as typed at the call sites before the header
static size_t ref_reduce(size_t n, size_t count, size_t ext) {
    return R(early_of(count, n) * ext + 16) * n + R(count * ext);
}
static size_t ref_rs(size_t n, size_t maxc, size_t ext) { return R(maxc * ext + 16) * (n + 1); }
static size_t ref_rs_inplace(size_t maxc, size_t ext) { return maxc * ext + 256; }
static size_t ref_scan(size_t bytes) { return bytes + 256; }
static size_t ref_push(size_t n, size_t count, size_t ext) { return R(early_of(count, n) * ext + 16) * n; }
static size_t ref_staged_push(size_t n, size_t count, size_t ext, bool want, bool *land) {
    const size_t slot = R(early_of(count, n) * ext + 16);
    *land = want && slot * (2 * n) <= kCap;
    return slot * (*land ? 2 * n : n + 1);
}
static size_t ref_ag_raw(size_t n, size_t bytes) { return R(bytes + 16) * n; }
static size_t ref_bcast_raw(size_t bytes) { return R(bytes) + 256; }
static size_t ref_a2a(size_t n, size_t chunk, size_t M) { return n * R(std::min(chunk, M) + 16); }
static size_t capped(size_t raw) { return raw + (64u << 20) > kCap ? 0 : raw; }

// the largest x in [0, hi] with f(x) <= limit (f is monotone)
static size_t largest(const std::function<size_t(size_t)> &f, size_t limit, size_t hi) {
    size_t lo = 0;
    if (f(0) > limit) return 0;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (f(mid) <= limit) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// result area inside need; the last input slot (any phase mod 16 B) before the result area
static void bounds(const char *what, const land_layout &L, size_t n_slots, size_t payload,
                   size_t result_bytes, size_t n, size_t count, size_t ext) {
    CHECK(L.result_off + result_bytes <= L.need, "%s n %zu count %zu ext %zu: result %zu + %zu > need %zu",
          what, n, count, ext, L.result_off, result_bytes, L.need);
    if (n_slots)
        CHECK((n_slots - 1) * L.slot + 15 + payload <= L.result_off,
              "%s n %zu count %zu ext %zu: slots end %zu > result_off %zu", what, n, count, ext,
              (n_slots - 1) * L.slot + 15 + payload, L.result_off);
}

static void check_one(size_t n, size_t ext, size_t count) {
    const int ni = (int)n;
    const size_t bytes = count * ext, early = early_of(count, n);
    CHECK(land_early(count, ni) == early, "n %zu count %zu", n, count);
    {
        const land_layout L = reduce_landing(ni, count, ext);
        CHECK(L.need == ref_reduce(n, count, ext), "reduce n %zu count %zu ext %zu: %zu", n, count, ext, L.need);
        bounds("reduce", L, n, early * ext, bytes, n, count, ext);
    }
    {
        const land_layout L = reduce_scatter_landing(ni, count, ext);  // count: the largest block
        CHECK(L.need == ref_rs(n, count, ext), "rs n %zu maxc %zu ext %zu: %zu", n, count, ext, L.need);
        bounds("reduce_scatter", L, n, bytes, 15 + bytes, n, count, ext);
        const land_layout I = reduce_scatter_inplace_landing(count, ext);
        CHECK(I.need == ref_rs_inplace(count, ext), "rs in place maxc %zu ext %zu: %zu", count, ext, I.need);
        bounds("reduce_scatter in place", I, 0, 0, bytes, n, count, ext);  // no input slots: the result alone
    }
    {
        const land_layout L = scan_landing(bytes);
        CHECK(L.need == ref_scan(bytes), "scan bytes %zu: %zu", bytes, L.need);
        bounds("scan", L, 1, bytes, 0, n, count, ext);
    }
    {
        const land_layout L = push_landing(ni, count, ext);
        CHECK(L.need == ref_push(n, count, ext), "push n %zu count %zu ext %zu: %zu", n, count, ext, L.need);
        bounds("push", L, n, early * ext, 0, n, count, ext);
    }
    for (int want = 0; want < 2; ++want) {
        bool land = false;
        const size_t need = ref_staged_push(n, count, ext, want != 0, &land);
        const land_layout L = staged_push_landing(ni, count, ext, want != 0);
        CHECK(L.need == need && L.land == land, "staged push n %zu count %zu ext %zu want %d: %zu land %d", n,
              count, ext, want, L.need, (int)L.land);
        // push-gather: result slot [n]; push-land: result slots [n, 2n)
        bounds("staged push", L, n, early * ext, (land ? (n - 1) * L.slot : 0) + 15 + early * ext, n, count, ext);
    }
    {
        const land_layout L = allgather_landing(ni, bytes);
        const size_t raw = ref_ag_raw(n, bytes);
        CHECK(L.need == capped(raw), "allgather n %zu bytes %zu: %zu", n, bytes, L.need);
        CHECK((L.need == 0) == (raw + (64u << 20) > kMaxIpcBytes), "allgather cap n %zu bytes %zu", n, bytes);
        if (L.need) bounds("allgather", L, n, bytes, 0, n, count, ext);
    }
    {
        const land_layout L = bcast_landing(ni, bytes);
        const size_t raw = ref_bcast_raw(bytes);
        CHECK(L.need == capped(raw), "bcast n %zu bytes %zu: %zu", n, bytes, L.need);
        CHECK((L.need == 0) == (raw + (64u << 20) > kMaxIpcBytes), "bcast cap n %zu bytes %zu", n, bytes);
        CHECK(L.blk == R((bytes + n - 1) / n) && L.blk == bcast_block(ni, bytes) && L.blk * n >= bytes,
              "bcast blk n %zu bytes %zu: %zu", n, bytes, L.blk);
        if (L.need) bounds("bcast", L, 1, bytes, 0, n, count, ext);
    }
    for (size_t chunk : {(size_t)1, (size_t)4096, (size_t)1 << 20, ~(size_t)0}) {  // the last: one pass
        const land_layout L = alltoall_landing(ni, chunk, bytes);
        CHECK(L.need == ref_a2a(n, chunk, bytes), "alltoall n %zu chunk %zu M %zu: %zu", n, chunk, bytes, L.need);
        bounds("alltoall", L, n, std::min(chunk, bytes), 0, n, count, ext);
    }
}

static void check_fit_chunk() {
    for (size_t n : {1, 2, 3, 4, 8, 16}) {
        // the default chunk: n slots under the allgather cap
        CHECK(alltoall_fit_chunk((int)n, kMaxIpcBytes - kLandCapMargin) ==
                  ((kCap - (64u << 20)) / n / 256 - 1) * 256, "default chunk n %zu", n);
        for (size_t avail : {(size_t)0, (size_t)511, (size_t)512 * n - 1, (size_t)512 * n, (size_t)4096 * n + 77,
                             kStepUsable, 2 * (kStepUsable + 64) - 64}) {
            const size_t per = (avail / n) & ~(size_t)255;
            const size_t fit = alltoall_fit_chunk((int)n, avail);
            CHECK(fit == (per < 512 ? 0 : per - 256), "fit n %zu avail %zu: %zu", n, avail, fit);
            if (fit) CHECK(alltoall_landing((int)n, fit, ~(size_t)0).need <= avail, "fit n %zu avail %zu", n, avail);
        }
    }
}

int main() {
    static_assert(kMaxIpcBytes == kCap, "IPC cap");
    for (size_t n : {1, 2, 3, 4, 8, 16})
        for (size_t ext : {1, 2, 4, 8, 16}) {
            std::vector<size_t> counts = {0, 1, n - 1, n, n + 1, 255, 256, 257, 1000003};
            // per scheme: the largest count whose need fits the first growth
            // step exactly, and one unit past it
            const size_t hi = (size_t)1 << 27;
            const std::function<size_t(size_t)> needs[] = {
                [&](size_t c) { return ref_reduce(n, c, ext); },
                [&](size_t c) { return ref_rs(n, c, ext); },
                [&](size_t c) { return ref_rs_inplace(c, ext); },
                [&](size_t c) { return ref_scan(c * ext); },
                [&](size_t c) { return ref_push(n, c, ext); },
                [&](size_t c) { bool l; return ref_staged_push(n, c, ext, false, &l); },
                [&](size_t c) { bool l; return ref_staged_push(n, c, ext, true, &l); },
                [&](size_t c) { return ref_ag_raw(n, c * ext); },
                [&](size_t c) { return ref_bcast_raw(c * ext); },
                [&](size_t c) { return ref_a2a(n, ~(size_t)0, c * ext); },
            };
            for (const auto &f : needs) {
                const size_t c = largest(f, kStepUsable, hi);
                counts.push_back(c);
                counts.push_back(c + 1);
            }
            // allgather / bcast: on and one past the IPC-cap fallback
            for (const auto &f : {needs[7], needs[8]}) {
                const size_t c = largest(f, kCap - (64u << 20), (size_t)1 << 32);
                counts.push_back(c);
                counts.push_back(c + 1);
            }
            {  // push-land: on and one past its fallback to push-gather (2n slots past the cap)
                const size_t c = largest([&](size_t k) { return R(early_of(k, n) * ext + 16) * 2 * n; }, kCap,
                                         (size_t)1 << 32);
                counts.push_back(c);
                counts.push_back(c + 1);
            }
            for (size_t count : counts) check_one(n, ext, count);
        }
    check_fit_chunk();
    if (failures) {
        fprintf(stderr, "%d landing layout checks failed\n", failures);
        return 1;
    }
    printf("landing layouts ok\n");
    return 0;
}
