// The HIP-free half of an event handle (cmf.jl_amd/csrc/cmf_events.h: the validation, the two orders of the index, the work tables) on the
// CPU, meant to be built with -fsanitize=address,undefined (tests/test_events_kl_cpu.py):
//   * lists with empty units, empty columns, ONE unit holding every event, T = 1, one event, and random ones;
//   * every refusal of cmf_events_validate, with its code;
//   * the index is checked against its definition: both pointer tables, the stable counting sort (units ascend within a column), the
//     permutation between the two orders, the sum of the counts;
//   * the work tables for chunk sizes 1, 2, 64 and "everything": the items of a destination tile its event range in order, a
//     destination with one chunk has slot -1, the others consecutive slots that their fix entry names.
// Prints "ok <lists> <refusals>" and exits 0, or a message and exits 1.
#include "cmf_events.h"

#include <cstdlib>
#include <limits>
#include <random>

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("line %d: %s does not hold\n", __LINE__, #cond);          \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

struct List {
    int64_t N, T;
    std::vector<int32_t> unit, time;
    std::vector<double> count;
};

static int validate(const List &e, int64_t K, int64_t L, std::string *msg)
{
    return cmf_events_validate(e.N, e.T, K, L, (int64_t)e.unit.size(), e.unit.data(), e.time.data(), e.count.data(), msg);
}

static void check_tables(const std::vector<int32_t> &ptr, int64_t ndest, int64_t window, int64_t chunk)
{
    std::vector<CmfEventsItem> items;
    std::vector<CmfEventsFix> fixes;
    const int64_t slots = cmf_events_items(ptr, ndest, window, chunk, &items, &fixes);
    size_t i = 0, f = 0;
    int64_t next_slot = 0;
    for (int64_t d = 0; d < ndest; ++d) {
        const int64_t b = ptr[(size_t)d], e = ptr[(size_t)std::min(d + window, ndest)];
        REQUIRE(i < items.size() && items[i].dest == d && items[i].begin == b);
        if (e - b <= chunk) {
            REQUIRE(items[i].end == e && items[i].slot == -1);
            ++i;
            continue;
        }
        REQUIRE(f < fixes.size() && fixes[f].dest == d && fixes[f].first == next_slot);
        int64_t at = b;
        for (int c = 0; c < fixes[f].n; ++c, ++i) {
            REQUIRE(i < items.size() && items[i].dest == d && items[i].begin == at && items[i].slot == next_slot + c);
            REQUIRE(items[i].end > items[i].begin && items[i].end - items[i].begin <= chunk);
            at = items[i].end;
        }
        REQUIRE(at == e);
        next_slot += fixes[f].n;
        ++f;
    }
    REQUIRE(i == items.size() && f == fixes.size() && next_slot == slots);
}

static void check_list(const List &e, int64_t L)
{
    std::string msg;
    REQUIRE(validate(e, 3, L, &msg) == 0);
    const int64_t nnz = (int64_t)e.unit.size();
    CmfEventsIndex ix;
    cmf_events_build_index(e.N, e.T, nnz, e.unit.data(), e.time.data(), e.count.data(), &ix);
    REQUIRE((int64_t)ix.unit_ptr.size() == e.N + 1 && (int64_t)ix.time_ptr.size() == e.T + 1);
    REQUIRE(ix.unit_ptr[0] == 0 && ix.unit_ptr[(size_t)e.N] == nnz && ix.time_ptr[0] == 0 && ix.time_ptr[(size_t)e.T] == nnz);
    double sum = 0.0;
    for (int64_t j = 0; j < nnz; ++j) {
        REQUIRE(ix.unit_ptr[(size_t)e.unit[j]] <= j && j < ix.unit_ptr[(size_t)e.unit[j] + 1]);
        REQUIRE(ix.um_time[(size_t)j] == e.time[j] && ix.um_count[(size_t)j] == (float)e.count[j]);
        sum += (double)(float)e.count[j];
    }
    REQUIRE(sum == ix.count_sum);
    std::vector<char> seen((size_t)nnz, 0);
    for (int64_t t = 0; t < e.T; ++t)
        for (int32_t p = ix.time_ptr[(size_t)t]; p < ix.time_ptr[(size_t)t + 1]; ++p) {
            const int32_t j = ix.tm_src[(size_t)p];
            REQUIRE(j >= 0 && j < nnz && !seen[(size_t)j]);
            seen[(size_t)j] = 1;
            REQUIRE(ix.tm_time[(size_t)p] == t && e.time[(size_t)j] == t && ix.tm_unit[(size_t)p] == e.unit[(size_t)j]);
            REQUIRE(ix.tm_count[(size_t)p] == (float)e.count[(size_t)j]);
            if (p > ix.time_ptr[(size_t)t]) REQUIRE(ix.tm_unit[(size_t)p] > ix.tm_unit[(size_t)p - 1]); // stable: units ascend
        }
    for (int64_t chunk : {(int64_t)1, (int64_t)2, (int64_t)64, nnz + 1}) {
        check_tables(ix.unit_ptr, e.N, 1, chunk);
        check_tables(ix.time_ptr, e.T, L, chunk);
    }
}

static List random_list(std::mt19937 &rng, int64_t N, int64_t T, double density, bool one_unit)
{
    List e{N, T, {}, {}, {}};
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const int64_t only = (int64_t)(rng() % (uint64_t)N);
    for (int64_t n = 0; n < N; ++n)
        for (int64_t t = 0; t < T; ++t)
            if (one_unit ? n == only : u(rng) < density) {
                e.unit.push_back((int32_t)n);
                e.time.push_back((int32_t)t);
                e.count.push_back(1.0 + (double)(rng() % 7) + 0.25 * u(rng));
            }
    if (e.unit.empty()) {
        e.unit.push_back((int32_t)only);
        e.time.push_back(0);
        e.count.push_back(2.0);
    }
    return e;
}

int main()
{
    std::mt19937 rng(2024);
    int lists = 0, refusals = 0;
    for (int rep = 0; rep < 40; ++rep) {
        check_list(random_list(rng, 1 + rng() % 9, 1 + rng() % 40, 0.05 + 0.1 * (rep % 5), false), 1 + rng() % 6); // empty units and columns
        check_list(random_list(rng, 1 + rng() % 9, 1 + rng() % 200, 0.0, true), 1 + rng() % 6);                 // one unit holds every event
        check_list(random_list(rng, 1 + rng() % 20, 1, 0.5, false), 1 + rng() % 6);                             // T = 1
        lists += 3;
    }
    check_list(List{5, 7, {3}, {6}, {1.5}}, 10); // one event, T < L
    check_list(random_list(rng, 70, 300, 0.3, false), 12);
    lists += 2;

    // refusals: every one names its reason, none reads past the arrays
    const List good{4, 6, {0, 0, 2, 3}, {1, 5, 0, 5}, {1.0, 2.0, 3.0, 4.0}};
    std::string msg;
    auto refused = [&](List e, int64_t K, int64_t L, int code) {
        msg.clear();
        REQUIRE(validate(e, K, L, &msg) == code && !msg.empty());
        ++refusals;
    };
    REQUIRE(validate(good, 3, 2, &msg) == 0);
    List e = good; e.unit[2] = 4; refused(e, 3, 2, 1);                                  // unit out of range
    e = good; e.unit[0] = -1; refused(e, 3, 2, 1);
    e = good; e.time[1] = 6; refused(e, 3, 2, 1);                                       // time out of range
    e = good; e.time[2] = -1; refused(e, 3, 2, 1);
    e = good; e.count[3] = 0.0; refused(e, 3, 2, 1);                                    // counts: zero, negative, NaN, infinite, too small / large for fp32
    e = good; e.count[0] = -1.0; refused(e, 3, 2, 1);
    e = good; e.count[1] = std::numeric_limits<double>::quiet_NaN(); refused(e, 3, 2, 1);
    e = good; e.count[1] = std::numeric_limits<double>::infinity(); refused(e, 3, 2, 1);
    e = good; e.count[1] = 1e-60; refused(e, 3, 2, 1);
    e = good; e.count[1] = 1e60; refused(e, 3, 2, 1);
    e = good; e.time[1] = 1; refused(e, 3, 2, 1);                                       // a duplicate
    e = good; std::swap(e.unit[2], e.unit[3]); refused(e, 3, 2, 1);                     // not sorted by unit
    e = good; std::swap(e.time[0], e.time[1]); refused(e, 3, 2, 1);                     // not sorted by time within a unit
    e = good; e.N = 0; refused(e, 3, 2, 1);
    e = good; e.T = 0; refused(e, 3, 2, 1);
    refused(good, 0, 2, 1);
    refused(good, 3, 0, 1);
    refused(List{4, 6, {}, {}, {}}, 3, 2, 1);                                           // nnz < 1
    msg.clear();
    REQUIRE(cmf_events_validate(4, 6, 3, 2, 4, nullptr, good.time.data(), good.count.data(), &msg) == 1 && !msg.empty());
    REQUIRE(cmf_events_validate(4, 6, 3, 2, 4, good.unit.data(), nullptr, good.count.data(), &msg) == 1);
    REQUIRE(cmf_events_validate(4, 6, 3, 2, 4, good.unit.data(), good.time.data(), nullptr, &msg) == 1);
    refusals += 3;
    refused(good, 257, 1, 4);                                                           // the limits, named
    REQUIRE(msg.find("256") != std::string::npos);
    refused(good, 33, 65, 4);
    REQUIRE(msg.find("4096") != std::string::npos);
    REQUIRE(validate(good, 33, 40, &msg) == 0 && validate(good, 256, 16, &msg) == 0 && validate(good, 32, 128, &msg) == 0);
    printf("ok %d %d\n", lists, refusals);
    return 0;
}
