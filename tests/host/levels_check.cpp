// Stand-alone check of elliot_amd/csrc/el_levels.h (plain C++, no GPU): built with -fsanitize=address,undefined and run by
// tests/test_levels_host.py.  Every array is sized exactly, so a read or write past an end is a sanitizer report.  Exit status 0
// when every case holds.
#include "el_levels.h"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

typedef std::vector<int32_t> I32;
typedef std::vector<int64_t> I64;

struct Result {
    int rc;
    int64_t bad, n_levels;
    I32 order;
    I64 start;          // the whole table of `cap` cells; -7 where nothing was written
};

// (i, j) on one item table, as el_bprslim_levels_host
static Result pairs(const I32& i, const I32& j, int64_t I, int64_t cap) {
    Result r{0, -1, -1, I32(i.size(), -7), I64((size_t)cap, -7)};
    r.rc = el_levels_build<0, 0>({i.data(), j.data()}, {I}, (int64_t)i.size(), r.order.data(), r.start.data(), cap, &r.n_levels,
                              &r.bad);
    return r;
}

// (u, i, j) on a user table and one item table, as el_bprsgd_levels_host
static Result triplets(const I32& u, const I32& i, const I32& j, int64_t U, int64_t I, int64_t cap) {
    Result r{0, -1, -1, I32(u.size(), -7), I64((size_t)cap, -7)};
    r.rc = el_levels_build<0, 1, 1>({u.data(), i.data(), j.data()}, {U, I}, (int64_t)u.size(), r.order.data(), r.start.data(),
                              cap, &r.n_levels, &r.bad);
    return r;
}

int main() {
    {   // n = 0: no level, level_start = [0]
        const Result r = pairs({}, {}, 4, 1);
        CHECK(r.rc == EL_LEVELS_OK && r.n_levels == 0 && r.start == I64({0}));
        const Result t = triplets({}, {}, {}, 3, 4, 1);
        CHECK(t.rc == EL_LEVELS_OK && t.n_levels == 0 && t.start == I64({0}));
    }
    {   // n = 1
        const Result r = pairs({2}, {3}, 4, 2);
        CHECK(r.rc == EL_LEVELS_OK && r.n_levels == 1 && r.order == I32({0}) && r.start == I64({0, 1}));
        const Result t = triplets({0}, {2}, {3}, 1, 4, 2);
        CHECK(t.rc == EL_LEVELS_OK && t.n_levels == 1 && t.order == I32({0}) && t.start == I64({0, 1}));
    }
    {   // every event on one row: n levels of one event, in sequence order
        const Result r = pairs({0, 0, 0, 0, 0}, {1, 2, 3, 4, 5}, 6, 6);
        CHECK(r.rc == EL_LEVELS_OK && r.n_levels == 5 && r.order == I32({0, 1, 2, 3, 4}) && r.start == I64({0, 1, 2, 3, 4, 5}));
        // the same items under one user; under five users the item pairs below share nothing and stand on one level
        const Result t = triplets({2, 2, 2, 2, 2}, {0, 2, 4, 6, 8}, {1, 3, 5, 7, 9}, 3, 10, 6);
        CHECK(t.rc == EL_LEVELS_OK && t.n_levels == 5 && t.order == I32({0, 1, 2, 3, 4}));
        const Result f = triplets({0, 1, 2, 3, 4}, {0, 2, 4, 6, 8}, {1, 3, 5, 7, 9}, 5, 10, 2);
        CHECK(f.rc == EL_LEVELS_OK && f.n_levels == 1 && f.order == I32({0, 1, 2, 3, 4}) && f.start == I64({0, 5}));
    }
    {   // i == j: one row, touched twice by one event
        const Result r = pairs({1, 1, 2}, {1, 0, 2}, 3, 4);
        CHECK(r.rc == EL_LEVELS_OK && r.n_levels == 2 && r.order == I32({0, 2, 1}) && r.start == I64({0, 2, 3, -7}));
    }
    {   // the user table and the item table are distinct: user 1 and item 1 share nothing
        const Result t = triplets({1, 0}, {0, 1}, {2, 3}, 2, 4, 3);
        CHECK(t.rc == EL_LEVELS_OK && t.n_levels == 1 && t.start == I64({0, 2, -7}));
    }
    {   // 0|1, 2|3 -> level 1; 0|2, 1|3 -> level 2; the sequence order inside a level
        const Result r = pairs({0, 2, 0, 1}, {1, 3, 2, 3}, 4, 6);
        CHECK(r.rc == EL_LEVELS_OK && r.n_levels == 2 && r.order == I32({0, 1, 2, 3}) && r.start == I64({0, 2, 4, -7, -7, -7}));
    }
    {   // capacity exactly maxl + 1, and one short: refused with the level count, nothing written
        const Result r = pairs({0, 0, 0}, {1, 1, 1}, 2, 4);
        CHECK(r.rc == EL_LEVELS_OK && r.n_levels == 3 && r.start == I64({0, 1, 2, 3}));
        const Result s = pairs({0, 0, 0}, {1, 1, 1}, 2, 3);
        CHECK(s.rc == EL_LEVELS_NO_ROOM && s.bad == 3 && s.start == I64({-7, -7, -7}) && s.order == I32({-7, -7, -7}));
    }
    {   // an id of -1, and an id equal to its table's size, at a known t
        CHECK(pairs({0, 1, -1}, {1, 2, 0}, 3, 5).rc == EL_LEVELS_BAD_ID && pairs({0, 1, -1}, {1, 2, 0}, 3, 5).bad == 2);
        CHECK(pairs({0, 1, 2}, {1, 3, 0}, 3, 5).rc == EL_LEVELS_BAD_ID && pairs({0, 1, 2}, {1, 3, 0}, 3, 5).bad == 1);
        const Result t = triplets({0, 2, 0}, {0, 1, 2}, {1, 2, 0}, 2, 3, 5);     // u = U; 2 is a good item
        CHECK(t.rc == EL_LEVELS_BAD_ID && t.bad == 1);
        const Result v = triplets({0, 1, 0}, {0, 1, 2}, {1, 2, 3}, 4, 3, 5);     // j = I; 3 is a good user
        CHECK(v.rc == EL_LEVELS_BAD_ID && v.bad == 2);
        CHECK(triplets({-1}, {0}, {1}, 2, 3, 5).rc == EL_LEVELS_BAD_ID && triplets({-1}, {0}, {1}, 2, 3, 5).bad == 0);
    }
    {   // el_levels_apply: empty levels are passed over, a launch's failure ends the loop, a malformed table launches nothing
        std::vector<I64> calls;
        int64_t bad = -1;
        const auto record = [&](int64_t first, int64_t n) {
            calls.push_back({first, n});
            return 0;
        };
        const I64 good = {0, 3, 3, 7};
        CHECK(el_levels_apply(good.data(), 3, &bad, record) == EL_LEVELS_OK && calls == std::vector<I64>({{0, 3}, {3, 4}}));
        calls.clear();
        CHECK(el_levels_apply(good.data(), 0, &bad, record) == EL_LEVELS_OK && calls.empty());
        const I64 back = {0, 3, 2, 7}, negative = {-1, 3, 4};
        CHECK(el_levels_apply(back.data(), 3, &bad, record) == EL_LEVELS_BAD_TABLE && bad == 1 && calls.empty());
        CHECK(el_levels_apply(negative.data(), 2, &bad, record) == EL_LEVELS_BAD_TABLE && bad == 0 && calls.empty());
        CHECK(el_levels_apply(good.data(), 3, &bad, [&](int64_t first, int64_t) { return first == 0 ? 5 : 0; }) == 5);
    }
    if (failures) return 1;
    std::printf("levels_check: ok\n");
    return 0;
}
