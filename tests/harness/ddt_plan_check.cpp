// Stand-alone check of ompi_amd/csrc/ddt_plan.h (tests/test_ddt_plan_cpu.py
// builds it with -fsanitize=address,undefined and runs it): for a set of
// layouts and every setting at both ends of its accepted range and at its
// default, a tile plan must fit a workgroup's LDS, hold at least one period,
// keep whole granules per period, and (unpack) stage no more packed bytes
// than its LDS data area holds.  Values just outside a range must be refused.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../ompi_amd/csrc/ddt_plan.h"

using namespace ompi_amd;

static int failures = 0;
static long plans = 0;
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

struct elem { int64_t count, blen, stride, disp; };
struct layout {
    std::string name;
    std::vector<elem> elems;
    int64_t extent;
};

static int gran_of(const layout &l) {
    uint64_t acc = (uint64_t)(l.extent < 0 ? -l.extent : l.extent);
    for (const auto &e : l.elems)
        acc |= (uint64_t)e.blen | (uint64_t)(e.disp < 0 ? -e.disp : e.disp) |
               (uint64_t)(e.stride < 0 ? -e.stride : e.stride);
    int g = 16;
    while (g > 1 && acc % (uint64_t)g) g >>= 1;
    return g;
}

static ddt_plan_type type_of(const layout &l) {
    ddt_plan_type t;
    t.nelem = l.elems.size();
    t.count0 = l.elems[0].count;
    t.blen0 = l.elems[0].blen;
    t.stride0 = l.elems[0].count > 1 ? l.elems[0].stride : l.elems[0].blen;
    t.disp0 = l.elems[0].disp;
    t.extent = l.extent;
    std::vector<std::pair<int64_t, int64_t>> runs;
    for (const auto &e : l.elems) {
        t.size += e.count * e.blen;
        t.max_blen = std::max(t.max_blen, e.blen);
        if (t.size <= kInstTileMaxSize)
            for (int64_t k = 0; k < e.count; ++k)
                runs.emplace_back(e.disp + k * e.stride, e.disp + k * e.stride + e.blen);
    }
    t.inst_tile = plan_inst_tile(runs, t.size, l.extent, &t.lo, &t.hi);
    return t;
}

static std::vector<layout> layouts() {
    std::vector<layout> v;
    // vectors of doubles: bl1, bl8, bl64 at gaps of 8, 64, 512 and 5000 B,
    // as one long instance and as many 5-run instances
    for (int64_t bl : {1, 8, 64})
        for (int64_t gap : {8, 64, 512, 5000}) {
            const int64_t b = 8 * bl, st = b + gap;
            v.push_back({"vector bl" + std::to_string(bl) + " gap " + std::to_string(gap),
                         {{300007, b, st, 0}}, 300006 * st + b});
            v.push_back({"vector5 bl" + std::to_string(bl) + " gap " + std::to_string(gap),
                         {{5, b, st, 0}}, 5 * st});
        }
    v.push_back({"struct{int,double}", {{1, 4, 4, 0}, {1, 8, 8, 8}}, 16});
    {   // blacs indexed of ints (tests/test_ddt_gpu.py)
        const int lens[] = {13, 13, 13, 13, 13, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1};
        const int disps[] = {286, 308, 330, 352, 374, 396, 419, 442, 465, 488, 511, 534, 557, 580,
                             603, 626, 649, 672};
        layout l{"blacs", {}, 673 * 4 - 286 * 4};
        for (int i = 0; i < 18; ++i) l.elems.push_back({1, lens[i] * 4, lens[i] * 4, disps[i] * 4});
        v.push_back(l);
    }
    {   // an 8 KiB instance: 1024 runs of 8 B at alternating gaps of 4 and 8 B
        layout l{"struct 8 KiB instance", {}, 0};
        int64_t pos = 0;
        for (int i = 0; i < 1024; ++i) {
            l.elems.push_back({1, 8, 8, pos});
            pos += 8 + (i % 2 ? 8 : 4);
        }
        l.extent = pos;
        v.push_back(l);
    }
    // the largest instance the byte map takes at the largest tile: 15 KiB
    // spanned, 8 KiB packed
    {
        layout l{"struct 15 KiB span", {}, 0};
        int64_t pos = 0;
        for (int i = 0; i < 512; ++i) {
            l.elems.push_back({1, 16, 16, pos});
            pos += 30;
        }
        l.extent = pos;
        v.push_back(l);
    }
    return v;
}

static void check_plan(const layout &l, const ddt_plan_type &t, size_t count, int G, bool unpack,
                       const ddt_knobs &k, const char *kn) {
    ddt_tile_plan P;
    if (!plan_tile_period(t, count, G, unpack, k, &P)) return;
    ++plans;
    const char *n = l.name.c_str();
    CHECK((int64_t)P.lds <= kLdsMaxBytes, "%s [%s] G=%d unpack=%d: lds %zu", n, kn, G, unpack, P.lds);
    CHECK(P.nper >= 1, "%s [%s] G=%d: nper %lld", n, kn, G, (long long)P.nper);
    CHECK(P.psize > 0 && P.psize % G == 0, "%s [%s] G=%d: psize %lld", n, kn, G, (long long)P.psize);
    CHECK(P.pext >= 0, "%s [%s]: pext %lld", n, kn, (long long)P.pext);
    const int64_t data = (int64_t)P.lds - P.map_bytes;
    // typed span of a tile at any 16-B phase
    CHECK((P.nper - 1) * P.pext + P.span + 15 + 15 <= data, "%s [%s] G=%d: span past the data area",
          n, kn, G);
    // unpack: the packed bytes of the tile's periods at any 16-B phase
    if (unpack)
        CHECK(P.nper * P.psize + 15 + 15 <= data, "%s [%s] G=%d: %lld periods of %lld B > %lld", n,
              kn, G, (long long)P.nper, (long long)P.psize, (long long)data);
    if (!P.ident) {
        CHECK(P.map_bytes >= 2 * P.psize, "%s [%s]: map %lld for %lld B", n, kn,
              (long long)P.map_bytes, (long long)P.psize);
        CHECK(P.span <= 65536, "%s [%s]: 16-bit map over %lld B", n, kn, (long long)P.span);
    }
}

// fdiv_q of ddt_device.h restated for the host (umulhi = the high word of
// the 64-bit product).
static uint32_t fdiv_q(uint32_t n, const fastdiv &f) {
    const uint32_t t = (uint32_t)(((uint64_t)n * f.m) >> 32);
    return (t + ((n - t) >> f.s1)) >> f.s2;
}

// make_fdiv + fdiv_q exact against integer division: 2^20 random n per
// divisor, and n = m*d - 1, m*d, m*d + 1 around the multiples of d — every
// multiple when there are at most 2^16 of them below 2^32, else the first
// and last 1024 and 2^16 spread evenly between (all 2^32 / d of a small d
// would take minutes).
static void check_fdiv() {
    std::vector<uint32_t> ds = {1, 2, 3, 5, 7, 0xFFFFFFFFu};
    for (int k = 0; k < 32; ++k) {
        const uint64_t p = 1ull << k;
        ds.push_back((uint32_t)p);
        if (p > 1) ds.push_back((uint32_t)(p - 1));
        ds.push_back((uint32_t)(p + 1));
    }
    uint64_t x = 0x9E3779B97F4A7C15ull;
    long checked = 0;
    for (uint32_t d : ds) {
        const fastdiv f = make_fdiv(d);
        auto one = [&](uint32_t n) {
            ++checked;
            CHECK(fdiv_q(n, f) == n / d, "fdiv %u / %u = %u", n, d, fdiv_q(n, f));
        };
        for (int i = 0; i < (1 << 20); ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;  // xorshift64
            one((uint32_t)(x >> 16));
        }
        const uint64_t nmul = (1ull << 32) / d;  // multiples m*d, m = 1 .. nmul, below or at 2^32
        auto around = [&](uint64_t m) {
            const uint64_t b = m * d;
            for (int64_t o = -1; o <= 1; ++o)
                if ((int64_t)b + o >= 0 && b + o < (1ull << 32)) one((uint32_t)(b + o));
        };
        if (nmul <= (1u << 16)) {
            for (uint64_t m = 0; m <= nmul; ++m) around(m);
        } else {
            for (uint64_t m = 0; m < 1024; ++m) { around(m); around(nmul - m); }
            for (uint64_t i = 0; i < (1u << 16); ++i) around(i * (nmul >> 16));
        }
        one(0);
        one(0xFFFFFFFFu);
    }
    if (!failures) printf("fdiv ok (%zu divisors, %ld quotients)\n", ds.size(), checked);
}

int main() {
    check_fdiv();
    // ranges: both ends accepted, one past each end refused (the default holds)
    CHECK(parse_tile_bytes("4096") == 4096 && parse_tile_bytes("61440") == 61440, "tile ends");
    CHECK(parse_tile_bytes("4095") == kTileDataDefault && parse_tile_bytes("61441") == kTileDataDefault,
          "tile outside");
    CHECK(parse_tile_bytes(nullptr) == kTileDataDefault, "tile unset");
    CHECK(parse_unpack_tile_bytes("1024") == 1024 && parse_unpack_tile_bytes("131072") == 131072,
          "unpack tile ends");
    CHECK(parse_unpack_tile_bytes("1023") == 0 && parse_unpack_tile_bytes("131073") == 0 &&
              parse_unpack_tile_bytes("1048576") == 0 && parse_unpack_tile_bytes(nullptr) == 0,
          "unpack tile outside");
    CHECK(parse_run_max_gap("-5") == 0 && parse_run_max_gap(nullptr) == 4096, "run gap");
    CHECK(parse_tile_off("0") && !parse_tile_off("1") && !parse_tile_off(nullptr), "tile off");
    CHECK(!parse_tile_wide("0") && parse_tile_wide("1") && parse_tile_wide(nullptr), "tile wide");
    CHECK(parse_unpack_nt(nullptr) == -1 && parse_unpack_nt("0") == 0 && parse_unpack_nt("1") == 1, "nt");

    const char *tile_bytes[] = {nullptr, "4096", "61440"};
    const char *unpack_bytes[] = {nullptr, "1024", "131072"};
    const char *wide[] = {nullptr, "0", "1"};
    const char *nt[] = {nullptr, "0", "1"};
    const char *gap[] = {nullptr, "0", "128", "1099511627776"};
    const auto all = layouts();
    for (const auto &l : all) {
        const ddt_plan_type t = type_of(l);
        const int g0 = gran_of(l);
        for (const char *tb : tile_bytes)
            for (const char *ub : unpack_bytes)
                for (const char *w : wide)
                    for (const char *n : nt)
                        for (const char *g : gap) {
                            const ddt_knobs k = knobs_from(nullptr, w, tb, ub, n, g);
                            char kn[160];
                            snprintf(kn, sizeof kn, "tile %s unpack %s wide %s nt %s gap %s",
                                     tb ? tb : "-", ub ? ub : "-", w ? w : "-", n ? n : "-", g ? g : "-");
                            for (int G = g0; G >= 1; G >>= 1)
                                for (size_t count : {(size_t)1, (size_t)4001})
                                    for (int unpack = 0; unpack < 2; ++unpack)
                                        check_plan(l, t, count, G, unpack != 0, k, kn);
                        }
        // OMPI_AMD_DDT_TILE=0: no plan at all
        ddt_tile_plan P;
        CHECK(!plan_tile_period(t, 1, g0, false, knobs_from("0", nullptr, nullptr, nullptr, nullptr, nullptr), &P),
              "%s: a plan with the tile off", l.name.c_str());
    }
    // the default settings do plan the layouts the tile was built for, and
    // the largest tile plans the 8 KiB instance (the largest byte map)
    {
        ddt_tile_plan P;
        const ddt_knobs k;
        const ddt_knobs big = knobs_from(nullptr, nullptr, "61440", "131072", nullptr, nullptr);
        for (const auto &l : all) {
            const bool dflt = l.name == "struct{int,double}" || l.name == "blacs" || l.name == "vector bl1 gap 8";
            if (!dflt && l.name != "struct 8 KiB instance") continue;
            const size_t count = l.elems.size() == 1 ? 1 : 4001;
            for (int unpack = 0; unpack < 2; ++unpack) {
                CHECK(plan_tile_period(type_of(l), count, gran_of(l), unpack != 0, dflt ? k : big, &P),
                      "%s unpack=%d: no plan", l.name.c_str(), unpack);
                if (!dflt) CHECK(P.map_bytes == 16384, "map of %lld B", (long long)P.map_bytes);
            }
        }
    }
    // the range OMPI_AMD_DDT_UNPACK_TILE_BYTES had (up to 1 MiB), handed
    // past the parser: its LDS request is over a workgroup's, so no plan
    {
        ddt_knobs k;
        k.unpack_tile_bytes = 1 << 20;
        ddt_tile_plan P;
        CHECK(!plan_tile_period(type_of(all[0]), 1, 8, true, k, &P), "a 1 MiB unpack tile planned");
        k.unpack_tile_bytes = 163840;
        CHECK(!plan_tile_period(type_of(all[0]), 1, 8, true, k, &P), "a 160 KiB unpack tile planned");
    }
    CHECK(plans > 1000, "only %ld plans checked", plans);
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("ddt plans ok (%ld plans)\n", plans);
    return 0;
}
