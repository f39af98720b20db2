/*
 * tracker_plan_main.cpp -- walks the two pure host headers of the multi-stream tracker without a device: the tick plan
 * (rgbd_odometry_amd/csrc/dvo_tracker_plan.h) and the key-frame ring rule (rgbd_odometry_amd/csrc/dvo_key_ring.h).
 * Stand-alone: built (plainly and under the address and undefined-behaviour sanitizers) and run by tests/test_tracker_plan_cpu.py.
 *
 * Both are checked against deliberately naive restatements written here, never against themselves.  The plan: per-stream scans
 * instead of a sort and a run cutter.  The ring: the whole history of candidates, replayed from scratch after every call into a map
 * from slot to its last writer (an array of three); what is live, evicted, written, and every counter is read off that replay.
 * Prints "ok <plan cases> <ring calls>".
 */
#include "dvo_key_ring.h"
#include "dvo_tracker_plan.h"

#include <cstdio>

using namespace dvo_host;

namespace {

long g_failed = 0;

void fail(int line, const char *what) {
    if (g_failed++ < 20) std::fprintf(stderr, "tracker_plan_main.cpp:%d: %s\n", line, what);
}
#define CHECK(cond) do { if (!(cond)) fail(__LINE__, #cond); } while (0)

/* ---- the tick plan ------------------------------------------------------------------------------------------------------------ */
constexpr int K = 4;

/* the runs of plan entries `set` as one number per position: entries of one run share it */
std::vector<int> run_ids(const StepPlan &p, const std::vector<int> &set, bool by_bank) {
    std::vector<int> id(set.size(), -1);
    int n = 0;
    for_runs(set, p.stream_of, p.bank_of, by_bank, [&](size_t a, size_t b) {
        for (size_t k = a; k < b; k++) id[k] = n;
        n++;
        return DVO_OK;
    });
    return id;
}

void check_plan(const std::vector<StreamClock> &clk, const std::vector<int> &streams, long every) {
    const int count = (int)streams.size();
    const StepPlan p = plan_step(clk, count, streams.data(), every);
    /* banks: the other bank for a running stream; first frames go where most running streams of this tick write, bank 0 on a tie */
    int writers[2] = {0, 0};
    for (int s : streams)
        if (clk[s].started) writers[clk[s].bank == 0 ? 1 : 0]++;
    const int join = writers[1] > writers[0] ? 1 : 0;
    CHECK((int)p.stream_of.size() == count && (int)p.bank_of.size() == count);
    for (int i = 0; i < count; i++) {
        CHECK(p.stream_of[i] == streams[i]);
        CHECK(p.bank_of[i] == (clk[streams[i]].started ? (clk[streams[i]].bank == 0 ? 1 : 0) : join));
    }
    /* order, first, align: stream by stream */
    std::vector<int> order, first, align;
    for (int s = 0; s < K; s++)
        for (int i = 0; i < count; i++)
            if (streams[i] == s) {
                order.push_back(i);
                (clk[s].started ? align : first).push_back(i);
            }
    CHECK(p.order == order && p.first == first && p.align == align);
    /* upload runs: a new run wherever the stream is not the previous one's successor or the bank changes */
    std::vector<int> up(order.size(), -1);
    int n_up = 0;
    for (size_t k = 0; k < order.size(); k++) {
        if (k > 0 && (streams[order[k]] != streams[order[k - 1]] + 1 || p.bank_of[order[k]] != p.bank_of[order[k - 1]])) n_up++;
        up[k] = n_up;
    }
    std::vector<int> got(order.size(), -1);
    size_t at = 0;
    for (size_t q = 0; q < p.upload_runs.size(); q++) {
        CHECK(p.upload_runs[q].first == at && p.upload_runs[q].second > at && p.upload_runs[q].second <= order.size());
        for (size_t k = p.upload_runs[q].first; k < p.upload_runs[q].second && k < got.size(); k++) got[k] = (int)q;
        at = p.upload_runs[q].second;
    }
    CHECK(at == order.size() && got == up);
    CHECK(run_ids(p, p.order, true) == up);
    /* alignment runs of the one-point-per-lane path: gaps only */
    std::vector<int> al(align.size(), -1);
    int n_al = 0;
    for (size_t k = 0; k < align.size(); k++) {
        if (k > 0 && streams[align[k]] != streams[align[k - 1]] + 1) n_al++;
        al[k] = n_al;
    }
    CHECK(run_ids(p, p.align, false) == al);
    /* flags */
    CHECK(p.flags.size() == align.size());
    for (size_t k = 0; k < align.size() && k < p.flags.size(); k++) {
        const StreamClock &S = clk[streams[align[k]]];
        const long since = S.n_frame - S.last_ref;
        CHECK(p.flags[k] == ((since == every ? PLAN_TRK_FORCED : 0) | (since != 1 ? PLAN_TRK_MAY_SWITCH : 0)));
    }
}

long walk_plans() {
    long cases = 0;
    /* every subset and order of the K streams x every combination of started / not started and bank 0 / 1 */
    std::vector<std::vector<int>> lists;
    std::vector<int> cur;
    std::vector<char> used(K, 0);
    struct Rec {
        static void go(std::vector<std::vector<int>> &out, std::vector<int> &cur, std::vector<char> &used) {
            if (!cur.empty()) out.push_back(cur);
            for (int s = 0; s < K; s++)
                if (!used[s]) { used[s] = 1; cur.push_back(s); go(out, cur, used); cur.pop_back(); used[s] = 0; }
        }
    };
    Rec::go(lists, cur, used);
    CHECK(lists.size() == 64);
    for (int state = 0; state < 256; state++) {
        std::vector<StreamClock> clk(K);
        for (int s = 0; s < K; s++) {
            const int v = (state >> (2 * s)) & 3;
            clk[s].bank = v & 1;
            if (v & 2) { clk[s].started = true; clk[s].n_frame = 3 + s; clk[s].last_ref = s; }      /* since = 3: FORCED at every = 3 only */
        }
        for (const std::vector<int> &l : lists) { check_plan(clk, l, 5); cases++; }
    }
    /* the named cases, spelled out */
    {
        std::vector<StreamClock> clk(K);
        clk[0].first_frame(0); clk[1].first_frame(1);
        const int all[4] = {0, 1, 2, 3};
        const StepPlan tie = plan_step(clk, 4, all, 5);                      /* one stream writes bank 1, one bank 0: a tie */
        CHECK(tie.bank_of[0] == 1 && tie.bank_of[1] == 0 && tie.bank_of[2] == 0 && tie.bank_of[3] == 0);
        clk[1].bank = 0; clk[3].first_frame(1);
        const StepPlan late = plan_step(clk, 4, all, 5);                     /* two write bank 1, one bank 0: stream 2 joins the two */
        CHECK(late.bank_of[2] == 1 && late.first == std::vector<int>{2} && (late.align == std::vector<int>{0, 1, 3}));
        CHECK(late.upload_runs.size() == 2 && late.upload_runs[0].second == 3);      /* 0 1 2 in bank 1, then 3 in bank 0 */
        CHECK((run_ids(late, late.align, false) == std::vector<int>{0, 0, 1}));      /* 0 1 | 3: the gap, whatever the bank */
        const int gap[2] = {2, 0};
        clk[2].first_frame(0);
        const StepPlan g = plan_step(clk, 2, gap, 5);
        CHECK(g.order == (std::vector<int>{1, 0}) && g.upload_runs.size() == 2);
        clk[0].bank = 0; clk[1].bank = 1;
        const int two[2] = {0, 1};
        const StepPlan b = plan_step(clk, 2, two, 5);                        /* neighbours in different banks: two uploads, one alignment run */
        CHECK(b.upload_runs.size() == 2 && (run_ids(b, b.align, false) == std::vector<int>{0, 0}));
        cases += 4;
    }
    /* flags over n_frame - last_ref in 0 .. every + 1 */
    for (long every : {1L, 2L, 5L})
        for (long since = 0; since <= every + 1; since++)
            for (long base : {0L, 3L, 1000000L}) {
                std::vector<StreamClock> clk(K);
                clk[1].first_frame(1);
                clk[1].last_ref = base; clk[1].n_frame = base + since;
                const int one[1] = {1};
                const StepPlan p = plan_step(clk, 1, one, every);
                CHECK(p.flags.size() == 1);
                if (p.flags.size() == 1) {
                    CHECK(((p.flags[0] & PLAN_TRK_FORCED) != 0) == (since == every));
                    CHECK(((p.flags[0] & PLAN_TRK_MAY_SWITCH) != 0) == (clk[1].last_ref != clk[1].n_frame - 1));
                    CHECK((p.flags[0] & ~(PLAN_TRK_FORCED | PLAN_TRK_MAY_SWITCH)) == 0);
                }
                check_plan(clk, {1}, every);
                cases++;
            }
    /* the clock's two transitions */
    for (int event = 0; event <= 3; event++)
        for (int bank = 0; bank <= 1; bank++) {
            StreamClock c;
            CHECK(!c.started && c.n_frame == 0 && c.last_ref == 0 && c.bank == -1);
            c.n_frame = 9; c.last_ref = 4;
            c.first_frame(bank);
            CHECK(c.started && c.n_frame == 1 && c.last_ref == 0 && c.bank == bank);
            c.n_frame = 7; c.last_ref = 3;
            c.aligned_frame(event, 1 - bank);
            CHECK(c.started && c.n_frame == 8 && c.last_ref == (event >= 2 ? 6 : 3) && c.bank == 1 - bank);
            cases++;
        }
    return cases;
}

/* ---- the ring ----------------------------------------------------------------------------------------------------------------- */
constexpr int STREAMS = 3;

/* every candidate a ring has ever been given, in order; frame = its position here, so that a slot's record names its candidate */
struct Cand { bool fits; int stream; };
constexpr int MAX_HISTORY = 3 * 7 + 3;             /* three calls of up to 2 * 3 + 1 candidates, and the call after off-and-on */
struct Model {
    int capacity = 0;
    long long first_id = 0;                        /* ids go on from an earlier configuration */
    Cand history[MAX_HISTORY];
    int n_history = 0;
    /* replayed: */
    long long writer[3];                           /* slot -> id of its last writer, -1: none */
    int cand_of[MAX_HISTORY];                      /* id - first_id -> position in history */
    long long next = 0, archived = 0, refused = 0;
    void replay() {
        for (long long &w : writer) w = -1;
        next = first_id; archived = refused = 0;
        for (int h = 0; h < n_history; h++) {
            if (!history[h].fits) { refused++; continue; }
            writer[next % capacity] = next;
            cand_of[next - first_id] = h;
            next++; archived++;
        }
    }
    int n_live() const { return (writer[0] >= 0) + (writer[1] >= 0) + (writer[2] >= 0); }
    bool live(long long id) const { return id >= 0 && (writer[0] == id || writer[1] == id || writer[2] == id); }
    long long id_of(int h) const {
        for (long long id = first_id; id < next; id++) if (cand_of[id - first_id] == h) return id;
        return -1;
    }
    long long key_of(int stream) const {           /* the stream's last candidate decides: refused or evicted leaves it without */
        for (int h = n_history; h-- > 0;)
            if (history[h].stream == stream) return live(id_of(h)) ? id_of(h) : -1;
        return -1;
    }
};

bool same_ring(const KeyRing &a, const KeyRing &b) {
    if (a.capacity != b.capacity || a.next_id != b.next_id || a.n_archived != b.n_archived || a.n_refused != b.n_refused ||
        a.n_evicted != b.n_evicted || a.key_id != b.key_id || a.slot.size() != b.slot.size())
        return false;
    for (size_t s = 0; s < a.slot.size(); s++)
        if (a.slot[s].id != b.slot[s].id || a.slot[s].frame != b.slot[s].frame || a.slot[s].stream != b.slot[s].stream) return false;
    return true;
}

void check_ring(const KeyRing &ring, const Model &m) {
    CHECK(ring.capacity == m.capacity && ring.next_id == m.next);
    CHECK(ring.n_archived == m.archived && ring.n_refused == m.refused);
    CHECK(ring.n_evicted == m.archived - m.n_live());
    int slot = -7;
    CHECK(!ring.find(-1, &slot) && !ring.find(m.next, &slot) && !ring.find(m.next + 5, &slot) && slot == -7);      /* never given */
    for (long long id = 0; id < m.first_id; id++) CHECK(!ring.find(id));                    /* of an earlier configuration */
    for (long long id = m.first_id; id < m.next; id++) {
        slot = -7;
        const KeyRing::Meta *M = ring.find(id, &slot);
        if (!m.live(id)) { CHECK(!M && slot == -7); continue; }                             /* evicted */
        CHECK(M && slot >= 0 && slot < m.capacity && m.writer[slot] == id);
        if (M) CHECK(M->id == id && M->frame == m.cand_of[id - m.first_id] && M->stream == m.history[m.cand_of[id - m.first_id]].stream);
    }
    CHECK((int)ring.key_id.size() == STREAMS);
    for (int s = 0; s < STREAMS && s < (int)ring.key_id.size(); s++) CHECK(ring.key_id[(size_t)s] == m.key_of(s));
}

/* one call: n candidates, bit j of `refusals` = candidate j does not fit; streams cycle through imported (-1), 0, 1, 2 */
void one_call(KeyRing &ring, Model &m, int n, unsigned refusals, int depth) {
    const KeyRing before = ring;
    std::vector<char> fits((size_t)n);
    std::vector<KeyRing::Meta> meta((size_t)n);
    const int h0 = m.n_history;
    for (int j = 0; j < n; j++) {
        fits[(size_t)j] = !((refusals >> j) & 1);
        meta[(size_t)j].stream = (j + depth) % (STREAMS + 1) - 1;
        meta[(size_t)j].frame = h0 + j;
        m.history[m.n_history++] = Cand{fits[(size_t)j] != 0, meta[(size_t)j].stream};
    }
    const KeyRing::Plan plan = ring.plan(fits.data(), n);
    CHECK(same_ring(ring, before));                                          /* a plan changes nothing */
    m.replay();
    CHECK((int)plan.item.size() == n && plan.next_after == m.next);
    for (int j = 0; j < n && j < (int)plan.item.size(); j++) {
        const KeyRing::Planned &c = plan.item[(size_t)j];
        const long long id = m.id_of(h0 + j);
        CHECK(c.id == id && (id >= 0) == (fits[(size_t)j] != 0));
        CHECK(id < 0 ? c.slot == -1 : (c.slot >= 0 && c.slot < m.capacity && (m.live(id) ? m.writer[c.slot] == id : m.writer[c.slot] > id)));
        CHECK(c.written == (id >= 0 && m.live(id)));                         /* written, or overwritten by a later one of this call */
    }
    ring.commit(plan, meta.data());
    check_ring(ring, m);
}

long g_ring_calls = 0;

void walk_ring(const KeyRing &ring, const Model &m, int depth, int first_call_max) {
    if (depth == 3) return;
    const int max_n = depth == 0 ? first_call_max : 2 * m.capacity + 1;
    for (int n = 0; n <= max_n; n++)
        for (unsigned refusals = 0; refusals < (1u << n); refusals++) {
            KeyRing r = ring;
            Model mm = m;
            one_call(r, mm, n, refusals, depth);
            g_ring_calls++;
            if (depth == 0) {                                                /* off and on again: the ids go on counting, the rest starts again */
                KeyRing off = r;
                off.configure(0, 0);
                CHECK(off.capacity == 0 && off.next_id == r.next_id && !off.find(0) && !off.find(r.next_id - 1) && off.slot.empty());
                off.configure(2, STREAMS);
                Model again;
                again.capacity = 2; again.first_id = r.next_id;
                again.replay();
                check_ring(off, again);
                one_call(off, again, 3, 2u, 1);
            }
            walk_ring(r, mm, depth + 1, first_call_max);
        }
}

}  // namespace

int main() {
    const long plans = walk_plans();
    /* capacity 3: 255 kinds of call; the first call of a sequence stops at `capacity` candidates (every residue of the next id, the
     * ring empty to full), the other two are unrestricted -- three unrestricted ones are 16.6 M sequences, too slow under the sanitizers */
    for (int capacity = 1; capacity <= 3; capacity++) {
        KeyRing ring;
        ring.configure(capacity, STREAMS);
        Model m;
        m.capacity = capacity;
        m.replay();
        check_ring(ring, m);
        walk_ring(ring, m, 0, capacity == 3 ? capacity : 2 * capacity + 1);
    }
    if (g_failed) {
        std::fprintf(stderr, "%ld checks failed\n", g_failed);
        return 1;
    }
    std::printf("ok %ld %ld\n", plans, g_ring_calls);
    return 0;
}
