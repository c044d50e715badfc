// Host check of the contact-slot rule and the high-water-mark repair (mrp_world.h contact_slot_init,
// mrp_lane.h StateIO<ENV>::repair_marks: the arithmetic mrp_set_state runs before its upload).
// tests/test_lane_repair.py builds this with hipcc, host side only, and runs it.  Lanes are built by
// hand from the rule as this file restates it (cnext[c] = c + 1, the last slot NULLN, every other
// contact array 0) for the smallest layout (env 15, C = 14) and the granule unit's (env 2, C = 53).
// Prints one line per layout, "env<id> <failed> <checked>", and exits nonzero on any failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#define MRP_ENV 15   // the header wants one; the templates below are instantiated by id
#include "../gym_puzzles_amd/csrc/mrp_lane.h"

static_assert(contact_slot_init(0, 14) == 1u && contact_slot_init(13, 14) == 0xffffffffu && contact_slot_init(14, 14) == 0u,
              "the slot rule is a constant expression");

template <int ENV>
static int check(int want_c) {
    using IO = StateIO<ENV>;
    constexpr int C = IO::C, P = IO::P, NW = IO::NW, HWW = IO::HWW, NCA = LaneState<ENV>::NCA;
    constexpr uint32_t FILL = 0xa5a5a5a5u;   // the words outside the contact region: the repair must not touch them
    int bad = 0, n = 0;
    auto expect = [&](bool ok, const char* what, int a, int b) {
        ++n;
        if (!ok) { ++bad; std::printf("# env%d FAIL %s (%d, %d)\n", ENV, what, a, b); }
    };
    auto init = [](int a, int c) { return a == 0 ? (c + 1 < C ? (uint32_t)(c + 1) : 0xffffffffu) : 0u; };
    expect(C == want_c && NCA == 24 && HWW < P && P + NCA * C <= NW, "layout", C, P);

    // the slot rule: every index of array 0, and indices of other arrays
    for (int c = 0; c < C; ++c) expect(contact_slot_init(c, C) == init(0, c), "slot rule, array 0", c, 0);
    expect(contact_slot_init(C, C) == 0u, "slot rule, array 1 slot 0", C, 0);
    expect(contact_slot_init((NCA - 1) * C + C - 1, C) == 0u, "slot rule, last word", NCA * C - 1, 0);

    // `lanes` all-initial lanes with the stored mark `mark`
    auto fresh = [&](int lanes, int32_t mark) {
        std::vector<uint32_t> w((size_t)lanes * NW, FILL);
        for (int l = 0; l < lanes; ++l) {
            for (int a = 0; a < NCA; ++a)
                for (int c = 0; c < C; ++c) w[(size_t)l * NW + P + a * C + c] = init(a, c);
            w[(size_t)l * NW + HWW] = (uint32_t)mark;
        }
        return w;
    };
    // repairs `w`; true iff lane l's mark is `want` and no other word of any lane changed
    auto repaired = [&](std::vector<uint32_t> w, int lanes, int l, int32_t want) {
        const std::vector<uint32_t> before = w;
        IO::repair_marks(w.data(), (size_t)lanes);
        bool ok = (int32_t)w[(size_t)l * NW + HWW] == want;
        for (size_t i = 0; i < w.size(); ++i)
            if ((int)(i % NW) != HWW && w[i] != before[i]) ok = false;
        return ok;
    };

    expect(repaired(fresh(1, 0), 1, 0, 0), "all-initial lane", 0, 0);
    const int slots[3] = {0, 1, C - 1};
    for (int a = 0; a < NCA; ++a)
        for (int s : slots) {
            auto w = fresh(1, 0);
            w[P + a * C + s] ^= 1u;   // one non-initial word
            expect(repaired(w, 1, 0, s + 1), "one live word", a, s);
        }
    {
        auto w = fresh(1, 5);
        w[P + 3 * C + 1] = 7u;
        expect(repaired(w, 1, 0, 5), "stored mark above the found one is kept", 5, 2);
    }
    expect(repaired(fresh(1, C + 7), 1, 0, C), "stored mark above C is clamped", C + 7, 0);
    expect(repaired(fresh(1, INT32_MAX), 1, 0, C), "stored mark above C is clamped", INT32_MAX, 0);
    {
        auto w = fresh(1, C + 7);
        w[P + 0 * C + 2] = 0u;
        expect(repaired(w, 1, 0, C), "stored mark above C is clamped, live slots", C + 7, 3);
    }
    {
        auto w = fresh(1, -3);
        w[P + (NCA - 1) * C + 1] = 1u;
        expect(repaired(w, 1, 0, 2), "negative stored mark is raised to the found value", -3, 2);
    }
    expect(repaired(fresh(1, -3), 1, 0, 0), "negative stored mark, all-initial lane", -3, 0);
    {   // three lanes: each is repaired from its own words
        auto w = fresh(3, 0);
        w[(size_t)0 * NW + P + 5 * C + 2] = 9u;
        w[(size_t)2 * NW + P + 0 * C + (C - 1)] = 0u;
        expect(repaired(w, 3, 0, 3), "lane 0 of 3", 0, 3);
        expect(repaired(w, 3, 1, 0), "lane 1 of 3", 1, 0);
        expect(repaired(w, 3, 2, C), "lane 2 of 3", 2, C);
    }
    std::printf("env%d %d %d\n", ENV, bad, n);
    return bad;
}

int main() {
    const int bad = check<15>(14) + check<2>(53);
    return bad ? 1 : 0;
}
