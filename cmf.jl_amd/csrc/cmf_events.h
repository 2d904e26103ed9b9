// cmf_events.h -- the host side of an event list (cmf_events_create, include/cmf_hip.h), free of HIP so that the validation, the
// two orders of the index and the work tables can be run on a CPU under the sanitizers (tests/events_index_stress.cpp,
// tests/test_events_kl_cpu.py).
//
// An event is (unit n, time t, count x): one non-zero entry data[n, t] = x of the N x T matrix the KL form of the MU rule is fitted to.
// The list arrives sorted by (unit, time), strictly increasing.  The index holds it twice:
//   unit-major:  unit_ptr[N + 1], um_time, um_count                       -- the events of unit n are [unit_ptr[n], unit_ptr[n + 1])
//   time-major:  time_ptr[T + 1], tm_unit, tm_time, tm_count, tm_src      -- the events of column t are [time_ptr[t], time_ptr[t + 1]);
//                                                                            tm_src[p] is the unit-major position of time-major event p
// The time-major copy is a stable counting sort of the unit-major one: within a column the units ascend.
//
// Work tables (cmf_events_items): a destination -- a unit for numW, a column for numH -- owns a contiguous range of events.  A range of
// more than `chunk` events is cut into chunks of `chunk`; a destination with one chunk writes its sum where it belongs (slot -1), one
// with several writes partial sums to consecutive slots, which a second pass adds IN CHUNK ORDER (the `fixes` table): no atomics, and
// a few destinations with thousands of events do not serialise the launch.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// What the library refuses beyond the argument checks (CMF_ERR_UNSUPPORTED): the kernels keep W[:, n, :] of one unit in LDS and put the
// components on the lanes of at most one workgroup.
#define CMF_EVENTS_MAX_K 256          // components
#define CMF_EVENTS_MAX_LK 4096        // 32 * ceil(K / 32) * L: floats of W[:, n, :] in its padded layout (16 KB of LDS)

struct CmfEventsIndex {
    int64_t N = 0, T = 0, nnz = 0;
    std::vector<int32_t> unit_ptr, um_time;
    std::vector<float> um_count;
    std::vector<int32_t> time_ptr, tm_unit, tm_time, tm_src;
    std::vector<float> tm_count;
    double count_sum = 0.0; // the sum of the float roundings of the counts, in input order, in fp64 (what the dense rule sums of its fp32 data)
};

// One work item: events [begin, end) of destination `dest`; slot < 0: the only chunk of its destination.
struct CmfEventsItem {
    int32_t dest, begin, end, slot;
};
// A destination with several chunks: its partial sums are slots [first, first + n).
struct CmfEventsFix {
    int32_t dest, first, n, pad;
};

static inline std::string cmf_events_fmt(const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0)
{
    char buf[256];
    snprintf(buf, sizeof(buf), fmt, a, b, c, d);
    return buf;
}

// 0: the arguments describe an event list; 1: they do not (CMF_ERR_ARG), 4: they do, beyond what the kernels take (CMF_ERR_UNSUPPORTED).
// `msg` receives the reason.
static inline int cmf_events_validate(int64_t N, int64_t T, int64_t K, int64_t L, int64_t nnz, const int32_t *unit, const int32_t *time,
                                      const double *count, std::string *msg)
{
    if (N < 1 || T < 1 || K < 1 || L < 1) {
        *msg = cmf_events_fmt("N, T, K and L must be at least 1 (got N=%lld T=%lld K=%lld L=%lld)", N, T, K, L);
        return 1;
    }
    if (nnz < 1) {
        *msg = cmf_events_fmt("an event list needs at least one event (nnz=%lld)", nnz);
        return 1;
    }
    if (!unit || !time || !count) {
        *msg = "NULL argument: unit, time and count must each point to nnz entries";
        return 1;
    }
    if (N > (1 << 24) || T > (1 << 28) || K > 4096 || L > 4096) { // (the sizes the dense cmf_create takes)
        *msg = "problem size out of range";
        return 4;
    }
    if (nnz >= ((int64_t)1 << 31)) {
        *msg = cmf_events_fmt("nnz=%lld: the index holds event positions as 32-bit integers (fewer than 2^31 events)", nnz);
        return 4;
    }
    const int64_t K32 = (K + 31) / 32 * 32;
    if (K > CMF_EVENTS_MAX_K) {
        *msg = cmf_events_fmt("K=%lld: the event kernels put the components on the lanes of one workgroup (K <= %lld)", K, CMF_EVENTS_MAX_K);
        return 4;
    }
    if (K32 * L > CMF_EVENTS_MAX_LK) {
        *msg = cmf_events_fmt("K=%lld, L=%lld: the event kernels keep W[:, n, :] of one unit in LDS (32 * ceil(K / 32) * L <= %lld, got %lld)", K, L,
                              CMF_EVENTS_MAX_LK, K32 * L);
        return 4;
    }
    for (int64_t j = 0; j < nnz; ++j) {
        if (unit[j] < 0 || unit[j] >= N || time[j] < 0 || time[j] >= T) {
            *msg = cmf_events_fmt("event %lld: (unit %lld, time %lld) is outside the N x T matrix", j, unit[j], time[j]);
            return 1;
        }
        if (!(count[j] > 0.0) || !std::isfinite(count[j]) || !((float)count[j] > 0.f) || !std::isfinite((float)count[j])) {
            *msg = cmf_events_fmt("event %lld: counts must be finite and > 0 (in fp32 too)", j);
            return 1;
        }
        if (j > 0 && !(unit[j] > unit[j - 1] || (unit[j] == unit[j - 1] && time[j] > time[j - 1]))) {
            *msg = cmf_events_fmt("event %lld: events must be sorted by (unit, time), strictly increasing (no duplicates)", j);
            return 1;
        }
    }
    return 0;
}

// Both orders of a validated list.
static inline void cmf_events_build_index(int64_t N, int64_t T, int64_t nnz, const int32_t *unit, const int32_t *time, const double *count,
                                          CmfEventsIndex *ix)
{
    ix->N = N; ix->T = T; ix->nnz = nnz;
    ix->unit_ptr.assign((size_t)N + 1, 0);
    ix->time_ptr.assign((size_t)T + 1, 0);
    ix->um_time.resize((size_t)nnz);
    ix->um_count.resize((size_t)nnz);
    ix->tm_unit.resize((size_t)nnz);
    ix->tm_time.resize((size_t)nnz);
    ix->tm_src.resize((size_t)nnz);
    ix->tm_count.resize((size_t)nnz);
    ix->count_sum = 0.0;
    for (int64_t j = 0; j < nnz; ++j) {
        ix->unit_ptr[(size_t)unit[j] + 1] += 1;
        ix->time_ptr[(size_t)time[j] + 1] += 1;
        ix->um_time[(size_t)j] = time[j];
        ix->um_count[(size_t)j] = (float)count[j];
        ix->count_sum += (double)(float)count[j];
    }
    for (int64_t n = 0; n < N; ++n) ix->unit_ptr[(size_t)n + 1] += ix->unit_ptr[(size_t)n];
    for (int64_t t = 0; t < T; ++t) ix->time_ptr[(size_t)t + 1] += ix->time_ptr[(size_t)t];
    // the stable counting sort: events in unit-major order drop into their column's next free place
    std::vector<int32_t> next(ix->time_ptr.begin(), ix->time_ptr.end() - 1);
    for (int64_t j = 0; j < nnz; ++j) {
        const int32_t p = next[(size_t)time[j]]++;
        ix->tm_unit[(size_t)p] = unit[j];
        ix->tm_time[(size_t)p] = time[j];
        ix->tm_src[(size_t)p] = (int32_t)j;
        ix->tm_count[(size_t)p] = (float)count[j];
    }
}

// The work table of `ndest` destinations; destination d owns events [ptr[d], ptr[min(d + window, ndest)]) (window 1: the events of a
// unit; window L: the events numH of column d reads).  Returns the number of partial-sum slots.
static inline int64_t cmf_events_items(const std::vector<int32_t> &ptr, int64_t ndest, int64_t window, int64_t chunk, std::vector<CmfEventsItem> *items,
                                       std::vector<CmfEventsFix> *fixes)
{
    items->clear();
    fixes->clear();
    int64_t slots = 0;
    if (chunk < 1) chunk = 1;
    for (int64_t d = 0; d < ndest; ++d) {
        const int64_t b = ptr[(size_t)d], e = ptr[(size_t)(d + window < ndest ? d + window : ndest)];
        const int64_t nch = e - b <= chunk ? 1 : (e - b + chunk - 1) / chunk;
        if (nch == 1) {
            items->push_back({(int32_t)d, (int32_t)b, (int32_t)e, -1});
            continue;
        }
        fixes->push_back({(int32_t)d, (int32_t)slots, (int32_t)nch, 0});
        for (int64_t c = 0; c < nch; ++c) {
            const int64_t cb = b + c * chunk, ce = cb + chunk < e ? cb + chunk : e;
            items->push_back({(int32_t)d, (int32_t)cb, (int32_t)ce, (int32_t)(slots + c)});
        }
        slots += nch;
    }
    return slots;
}
