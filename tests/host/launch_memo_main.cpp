/*
 * launch_memo_main.cpp -- walks the key of enqueue()'s memo (rgbd_odometry_amd/csrc/dvo_launch_memo.h): equal keys hit, every
 * field of the key alone misses, a moved generation misses, and requests that must never be remembered are not.  Stand-alone:
 * built and run by tests/test_launch_memo_cpu.py.
 */
#include "dvo_launch_memo.h"

#include <cstdio>
#include <cstring>

using namespace dvo_host;

namespace {

int g_failed = 0;

void fail(int line, const char *what) {
    std::fprintf(stderr, "launch_memo_main.cpp:%d: %s\n", line, what);
    g_failed++;
}
#define CHECK(cond) do { if (!(cond)) fail(__LINE__, #cond); } while (0)

const int kIters[4] = {10, 10, 10, 10};

MemoKey base_key() {
    MemoKey k;
    k.q = memo_request(0, 40000, 4, kIters, 3, ~0u, 0, false);
    k.host_gen = 77; k.sched_gen = 2; k.final_cap = 15104; k.energy_size = 1600000; k.h_size = 0;
    return k;
}

/* a memo that remembered `k` */
LaunchMemo remembered(const MemoKey &k) {
    LaunchMemo m;
    m.record(k, MEMO_ON, 1, false, false);
    return m;
}

void expect_miss(int line, const MemoKey &changed, const char *field) {
    const LaunchMemo m = remembered(base_key());
    if (!m.valid) fail(line, "the base key was not remembered");
    if (m.matches(changed)) fail(line, "a changed key hit");
    const char *named = memo_key_mismatch(m.key, changed);
    if (!named || std::strcmp(named, field) != 0) {
        std::fprintf(stderr, "launch_memo_main.cpp:%d: mismatch named '%s', expected '%s'\n", line, named ? named : "(none)", field);
        g_failed++;
    }
}
#define EXPECT_MISS(key, field) expect_miss(__LINE__, key, field)

}  // namespace

int main() {
    /* the switch */
    CHECK(memo_mode(nullptr) == MEMO_ON && memo_mode("") == MEMO_ON && memo_mode("on") == MEMO_ON);
    CHECK(memo_mode("off") == MEMO_OFF && memo_mode("verify") == MEMO_VERIFY);
    CHECK(memo_mode("OFF") == MEMO_ON);                   /* anything else is the default */

    /* the request is held by value: iterations beyond n_levels do not count, a NULL schedule is all zeros */
    {
        const int six[6] = {1, 2, 3, 4, 5, 6};
        const MemoRequest r = memo_request(3, 5, 4, six, 1, ~0u, 0, false);
        CHECK(r.first_pair == 3 && r.n_pairs == 5 && r.n_levels == 4 && r.flags == 1);
        CHECK(r.iters[0] == 1 && r.iters[3] == 4 && r.iters[4] == 0 && r.iters[DVO_MAX_LEVELS - 1] == 0);
        const MemoRequest z = memo_request(0, 1, 4, nullptr, 0, ~0u, 0, false);
        for (int l = 0; l < DVO_MAX_LEVELS; l++) CHECK(z.iters[l] == 0);
    }

    /* nothing remembered: no hit */
    {
        LaunchMemo m;
        CHECK(!m.valid && !m.matches(base_key()));
    }
    /* equal keys hit, again and again; forget() ends it */
    {
        LaunchMemo m = remembered(base_key());
        CHECK(m.valid);
        CHECK(memo_key_mismatch(m.key, base_key()) == nullptr);
        CHECK(m.matches(base_key()) && m.matches(base_key()));
        MemoKey same = base_key();
        same.q = memo_request(0, 40000, 4, kIters, 3, ~0u, 0, false);      /* another array, the same schedule */
        CHECK(m.matches(same));
        m.forget();
        CHECK(!m.matches(base_key()));
    }
    /* each field of the key alone misses */
    { MemoKey k = base_key(); k.q.first_pair = 1; EXPECT_MISS(k, "first_pair"); }
    { MemoKey k = base_key(); k.q.n_pairs = 39999; EXPECT_MISS(k, "n_pairs"); }
    { MemoKey k = base_key(); k.q.n_levels = 3; EXPECT_MISS(k, "n_levels"); }
    for (int l = 0; l < DVO_MAX_LEVELS; l++) { MemoKey k = base_key(); k.q.iters[l] += 1; EXPECT_MISS(k, "iters"); }
    for (int bit = 0; bit < 4; bit++) { MemoKey k = base_key(); k.q.flags ^= 1 << bit; EXPECT_MISS(k, "flags"); }
    { MemoKey k = base_key(); k.q.level_mask = 0x3u; EXPECT_MISS(k, "level_mask"); }
    { MemoKey k = base_key(); k.q.forced_team = 32; EXPECT_MISS(k, "forced_team"); }
    { MemoKey k = base_key(); k.q.listed = true; EXPECT_MISS(k, "listed"); }
    { MemoKey k = base_key(); k.host_gen += 1; EXPECT_MISS(k, "host_gen"); }              /* a bumped generation */
    { MemoKey k = base_key(); k.host_gen -= 1; EXPECT_MISS(k, "host_gen"); }
    { MemoKey k = base_key(); k.sched_gen += 1; EXPECT_MISS(k, "sched_gen"); }
    { MemoKey k = base_key(); k.final_cap += 256; EXPECT_MISS(k, "final_cap"); }
    { MemoKey k = base_key(); k.energy_size *= 2; EXPECT_MISS(k, "energy_size"); }
    { MemoKey k = base_key(); k.h_size = 21 * k.energy_size; EXPECT_MISS(k, "h_size"); }

    /* what is never remembered */
    {
        const MemoKey k = base_key();
        CHECK(memo_recordable(k.q, 1, false, false));
        LaunchMemo m;
        m.record(k, MEMO_OFF, 1, false, false);  CHECK(!m.valid && !m.matches(k));       /* DVO_LAUNCH_MEMO=off */
        m.record(k, MEMO_VERIFY, 1, false, false); CHECK(m.valid && m.matches(k));
        m.record(k, MEMO_ON, 2, false, false);   CHECK(!m.valid && !m.matches(k));       /* a team launch (and it forgets the pass before) */
        m.record(k, MEMO_ON, 256, false, false); CHECK(!m.valid);
        m.record(k, MEMO_ON, 1, true, false);    CHECK(!m.valid);                        /* texels still to decode */
        m.record(k, MEMO_ON, 1, false, true);    CHECK(!m.valid);                        /* a compact build may come due */
        MemoKey listed = k;  listed.q.listed = true;
        m.record(listed, MEMO_ON, 1, false, false); CHECK(!m.valid && !m.matches(listed));
        MemoKey masked = k;  masked.q.level_mask = 0xeu;
        m.record(masked, MEMO_ON, 1, false, false); CHECK(!m.valid && !m.matches(masked));
        MemoKey forced = k;  forced.q.forced_team = 32;
        m.record(forced, MEMO_ON, 1, false, false); CHECK(!m.valid && !m.matches(forced));
        forced.q.forced_team = 1;                                                        /* forced to one workgroup is still a tier's launch */
        m.record(forced, MEMO_ON, 1, false, false); CHECK(!m.valid);
        CHECK(!memo_request_recordable(listed.q) && !memo_request_recordable(masked.q) && !memo_request_recordable(forced.q));
        m.record(k, MEMO_ON, 1, false, false);   CHECK(m.valid && m.matches(k));
    }
    /* a new recording replaces the old one */
    {
        LaunchMemo m = remembered(base_key());
        MemoKey other = base_key();
        other.q.n_pairs = 1024; other.host_gen = 90;
        m.record(other, MEMO_ON, 1, false, false);
        CHECK(m.matches(other) && !m.matches(base_key()));
    }
    /* the counters are the caller's to step; a recording leaves them alone */
    {
        LaunchMemo m;
        m.full_passes = 3; m.hits = 5;
        m.record(base_key(), MEMO_ON, 1, false, false);
        m.forget();
        CHECK(m.full_passes == 3 && m.hits == 5);
    }

    if (g_failed) { std::fprintf(stderr, "%d check(s) failed\n", g_failed); return 1; }
    std::printf("launch memo: ok\n");
    return 0;
}
