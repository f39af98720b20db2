/*
 * dvo_key_ring.h -- the host's side of the key-frame ring of the multi-stream tracker (dvo_tracker_set_archive): which id and slot a
 * new key frame gets, what it evicts, what the host knows of every slot, each stream's current key frame and the three counters.
 * The rule: ids never repeat (also across re-configurations); id lives in slot id % capacity; a candidate whose lists do not fit is
 * refused and counted; an occupied slot is evicted and counted, and streams whose key frame it was lose the id; when one call admits
 * more candidates than the ring has slots, the earlier ones are overwritten by the later ones and need not be written at all.
 * The step's store plans and commits at once; the import plans, waits for its checksums, then commits.
 * Host only, no HIP header: tests/host/tracker_plan_main.cpp walks it under a sanitizer.  Internal; not installed.
 */
#ifndef DVO_KEY_RING_H_
#define DVO_KEY_RING_H_

#include "../../include/dvo_amd.h"      /* DVO_MAX_LEVELS */

#include <cstddef>
#include <vector>

namespace dvo_host {

struct KeyRing {
    struct Meta {                                  /* what the host knows of a slot */
        long long id = -1;
        int stream = -1;                           /* -1: imported */
        long frame = 0;
        int N[DVO_MAX_LEVELS] = {};
        float K[4] = {};                           /* fx, fy, cx, cy: the bits the slot's header holds */
        bool has_desc = false;                     /* its place descriptor was stored with it (dvo_tracker_set_places) */
        long long origin_id = -1;                  /* who made it: itself, or -- imported -- what its blob recorded */
        int origin_stream = -1;
        long long origin_frame = 0;
    };
    struct Planned {
        long long id = -1;                         /* -1: refused */
        int slot = -1;
        bool written = false;                      /* admitted and not overwritten by a later candidate of the same call */
    };
    struct Plan {
        std::vector<Planned> item;                 /* one per candidate */
        long long next_after = 0;                  /* next_id once the plan is committed */
    };

    int capacity = 0;                              /* 0: the archive is off */
    long long next_id = 0;
    std::vector<Meta> slot;
    std::vector<long long> key_id;                 /* per stream: id of its current key frame, -1 = not archived */
    long long n_archived = 0, n_refused = 0, n_evicted = 0;

    /* an empty ring of `new_capacity` slots for `n_streams` streams (0, 0: off); the counters start again, the ids go on counting */
    void configure(int new_capacity, int n_streams) {
        const long long next = next_id;
        *this = KeyRing();
        next_id = next;
        capacity = new_capacity;
        slot.assign((size_t)new_capacity, Meta());
        key_id.assign((size_t)n_streams, -1);
    }

    /* the slot that holds `id`, or NULL (never given, refused, evicted, or the archive is off) */
    const Meta *find(long long id, int *slot_out = nullptr) const {
        if (capacity < 1 || id < 0 || id >= next_id) return nullptr;
        const int s = (int)(id % capacity);
        if (slot[(size_t)s].id != id) return nullptr;
        if (slot_out) *slot_out = s;
        return &slot[(size_t)s];
    }

    /* ids and slots of n candidates, fits[i] = its lists fit a slot; nothing changes.  Admitted ids are consecutive, so a later
     * candidate of the same call has the same slot exactly when id + capacity < next_after */
    Plan plan(const char *fits, int n) const {
        Plan p;
        p.item.resize((size_t)n);
        p.next_after = next_id;
        for (int i = 0; i < n; i++)
            if (fits[i]) {
                p.item[(size_t)i].id = p.next_after;
                p.item[(size_t)i].slot = (int)(p.next_after++ % capacity);
            }
        for (Planned &c : p.item) c.written = c.id >= 0 && !(c.id + capacity < p.next_after);
        return p;
    }

    /* the plan becomes the ring's state, candidate by candidate: meta[i] goes to its slot under its new id (a native key frame,
     * meta[i].stream >= 0, becomes its stream's; refused, it leaves the stream without one) */
    void commit(const Plan &p, const Meta *meta) {
        for (size_t i = 0; i < p.item.size(); i++) {
            const Planned &c = p.item[i];
            const int s = meta[i].stream;
            if (c.id < 0) {
                n_refused++;
                if (s >= 0) key_id[(size_t)s] = -1;
                continue;
            }
            Meta &M = slot[(size_t)c.slot];
            if (M.id >= 0) {
                n_evicted++;
                for (long long &k : key_id) if (k == M.id) k = -1;      /* a stream that still tracks against it keeps tracking; the id is gone */
            }
            M = meta[i];
            M.id = c.id;
            if (s >= 0) key_id[(size_t)s] = c.id;
            n_archived++;
        }
        next_id = p.next_after;
    }
};

}  // namespace dvo_host

#endif  // DVO_KEY_RING_H_
