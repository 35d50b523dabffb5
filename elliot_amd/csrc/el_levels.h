// Dependency levels of an event sequence, as plain C++ (no HIP): the scheduler behind el_bprsgd_levels_host and
// el_bprslim_levels_host, and the per-level launch loop behind the two *_apply_levels.
//
// An event reads and writes K rows: ids[r][t] names the row of table TAB[r] that event t touches through its r-th id; the tables
// are told apart at compile time, el_levels_build<0, 1, 1>({u, i, j}, {U, I}, ...).  An event stands one level above the last
// earlier event that shares a row with it, so the events of one level share no row and may run concurrently, and level after
// level reproduces the sequence.
#pragma once
#include <cstdint>
#include <vector>

enum { EL_LEVELS_OK = 0, EL_LEVELS_BAD_ID = -1, EL_LEVELS_NO_ROOM = -2, EL_LEVELS_BAD_TABLE = -3 };

// Level l (1-based) occupies order[level_start[l - 1] .. level_start[l]); within a level the sequence order is kept.
// EL_LEVELS_BAD_ID: *bad = the first event with an id outside its table; EL_LEVELS_NO_ROOM: *bad = the level count, which needs
// level_start_cap >= *bad + 1.  (static: the one caller of a translation unit inlines it and the loop gets that caller's code.)
template <int... TAB, int NT>
static int el_levels_build(const int32_t* const (&ids)[sizeof...(TAB)], const int64_t (&table_size)[NT], int64_t n, int32_t* order,
                    int64_t* level_start, int64_t level_start_cap, int64_t* n_levels, int64_t* bad) {
    constexpr int K = sizeof...(TAB), tab[K] = {TAB...};
    std::vector<int32_t> store[NT], lev(n);
    int32_t* last[NT];                                            // the level of the last event on every row of every table
    for (int a = 0; a < NT; ++a) store[a].assign(table_size[a], 0), last[a] = store[a].data();
    int32_t maxl = 0;
    for (int64_t t = 0; t < n; ++t) {
        int32_t id[K];                                            // read once: a store below may not make the compiler read again
        for (int r = 0; r < K; ++r) {
            id[r] = ids[r][t];
            if (id[r] < 0 || id[r] >= table_size[tab[r]]) {
                *bad = t;
                return EL_LEVELS_BAD_ID;
            }
        }
        int32_t l = last[tab[0]][id[0]];
        for (int r = 1; r < K; ++r)
            if (last[tab[r]][id[r]] > l) l = last[tab[r]][id[r]];
        lev[t] = ++l;
        for (int r = 0; r < K; ++r) last[tab[r]][id[r]] = l;
        if (l > maxl) maxl = l;
    }
    if ((int64_t)maxl + 1 > level_start_cap) {
        *bad = maxl;
        return EL_LEVELS_NO_ROOM;
    }
    std::vector<int64_t> count(maxl + 1, 0);
    for (int64_t t = 0; t < n; ++t) count[lev[t]]++;
    level_start[0] = 0;
    for (int32_t l = 1; l <= maxl; ++l) level_start[l] = level_start[l - 1] + count[l];
    std::vector<int64_t> cur(maxl + 1, 0);
    for (int32_t l = 1; l <= maxl; ++l) cur[l] = level_start[l - 1];
    for (int64_t t = 0; t < n; ++t) order[cur[lev[t]]++] = (int32_t)t;
    *n_levels = maxl;
    return EL_LEVELS_OK;
}

// launch(first, n) for every level that holds events, in order; its first non-zero result ends the loop and is returned.
// EL_LEVELS_BAD_TABLE: *bad = the first level that is not [a, b) with 0 <= a <= b; then nothing is launched.
template <class Launch>
static int el_levels_apply(const int64_t* level_start, int64_t n_levels, int64_t* bad, Launch&& launch) {
    for (int64_t L = 0; L < n_levels; ++L)
        if (!(level_start[L] >= 0 && level_start[L + 1] >= level_start[L])) {
            *bad = L;
            return EL_LEVELS_BAD_TABLE;
        }
    for (int64_t L = 0; L < n_levels; ++L) {
        const int64_t a = level_start[L], b = level_start[L + 1];
        if (b > a)
            if (int rc = launch(a, b - a)) return rc;
    }
    return EL_LEVELS_OK;
}
