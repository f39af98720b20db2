/*
 * now_state_main.cpp -- walks the transitions of dvo_host::NowState (rgbd_odometry_amd/csrc/dvo_now_state.h), the host's record of
 * one pair's now level, and checks every field after every step.  Stand-alone: built and run by tests/test_now_state_cpu.py.
 */
#include "dvo_now_state.h"

#include <cstdio>
#include <cstdlib>

using dvo_host::NowState;

namespace {

enum : char { UNKNOWN = NowState::P4_UNKNOWN, OK = NowState::P4_OK, REFUSED = NowState::P4_REFUSED, PARTIAL = NowState::P4_PARTIAL };
const int PN_OK = 300, PN_REFUSED = -2, PN_PARTIAL = NowState::PAL_PARTIAL_BIT | 4094;      /* what the device's pal_n can say */

int g_failed = 0;

void fail(int line, const char *what) {
    std::fprintf(stderr, "now_state_main.cpp:%d: %s\n", line, what);
    g_failed++;
}
#define CHECK(cond) do { if (!(cond)) fail(__LINE__, #cond); } while (0)

/* every field of the record */
void expect(int line, const NowState &s, int present, int uses, int built, int texels_stale, int known, int native, int fresh) {
    if (s.present != present || s.uses != uses || s.built != built || s.texels_stale != texels_stale || s.known != known ||
        s.native != native || s.fresh != fresh) {
        std::fprintf(stderr, "now_state_main.cpp:%d: {present %d uses %d built %d texels_stale %d known %d native %d fresh %d}, expected "
                             "{%d %d %d %d %d %d %d}\n", line, s.present, s.uses, s.built, s.texels_stale, s.known, s.native, s.fresh,
                     present, uses, built, texels_stale, known, native, fresh);
        g_failed++;
    }
}
#define EXPECT(s, ...) expect(__LINE__, s, __VA_ARGS__)

bool same(const NowState &a, const NowState &b) {
    return a.present == b.present && a.uses == b.uses && a.built == b.built && a.texels_stale == b.texels_stale && a.known == b.known &&
           a.native == b.native && a.fresh == b.fresh;
}

NowState native_compact(int pal_n) {      /* a natively written compact form whose pal_n the host has read back */
    NowState s;
    s.written_compact();
    s.learned(pal_n, false);
    return s;
}

}  // namespace

int main() {
    /*                 present uses built stale known native fresh */
    {   /* the defaults: what an empty per-pair vector used to answer */
        NowState s;
        EXPECT(s, 0, 0, 0, 0, UNKNOWN, 0, 0);
        CHECK(!s.ready() && s.texels_real() && !s.wants_build(false) && !s.wants_build(true) && !s.needs_readback(false) && !s.host_unknown());
        CHECK(sizeof(NowState) <= 12);
    }
    {   /* texel write, uses, build, refused read-back */
        NowState s;
        CHECK(!s.written_texels());
        EXPECT(s, 1, 0, 0, 0, UNKNOWN, 0, 0);
        CHECK(s.ready() && s.texels_real() && s.wants_build(false) && !s.wants_build(true));
        for (int u = 1; u <= DVO_COMPACT_NOW_AFTER + 1; u++) {
            s.used();
            EXPECT(s, 1, u, 0, 0, UNKNOWN, 0, 0);
            CHECK(s.wants_build(true) == (u >= DVO_COMPACT_NOW_AFTER));      /* flips exactly at DVO_COMPACT_NOW_AFTER */
            CHECK(s.wants_build(false));
        }
        NowState three;
        three.written_texels();
        three.used(); three.used(); three.used();
        EXPECT(three, 1, 3, 0, 0, UNKNOWN, 0, 0);
        CHECK(!three.wants_build(true) && three.wants_build(false));
        three.built_compact();
        EXPECT(three, 1, 3, 1, 0, UNKNOWN, 0, 0);
        CHECK(!three.wants_build(false) && !three.wants_build(true));
        CHECK(three.needs_readback(false) && three.needs_readback(true) && three.host_unknown());      /* the generic builder may refuse */
        CHECK(three.learned(PN_REFUSED, false));
        EXPECT(three, 1, 3, 1, 0, REFUSED, 0, 0);
        CHECK(three.texels_real() && !three.needs_readback(false) && !three.host_unknown());
    }
    {   /* native compact write with the three device answers */
        NowState s;
        s.written_compact();
        EXPECT(s, 1, 0, 1, 1, UNKNOWN, 1, 0);
        CHECK(s.ready() && !s.texels_real() && !s.wants_build(false));
        CHECK(!s.needs_readback(true) && s.needs_readback(false) && s.host_unknown());      /* never refused: the launch shape needs no read-back */
        NowState ok = s, refused = s, partial = s;
        CHECK(!ok.learned(PN_OK, false));
        EXPECT(ok, 1, 0, 1, 1, OK, 1, 0);
        CHECK(!ok.texels_real() && !ok.needs_readback(false));
        CHECK(refused.learned(PN_REFUSED, false));
        EXPECT(refused, 1, 0, 1, 0, REFUSED, 1, 0);
        CHECK(refused.texels_real() && !refused.needs_readback(false));
        CHECK(refused.learned(0, false));                  /* pal_n = 0 is "no compact form" too */
        EXPECT(refused, 1, 0, 1, 0, REFUSED, 1, 0);
        CHECK(partial.learned(PN_PARTIAL, false));
        EXPECT(partial, 1, 0, 1, 0, PARTIAL, 1, 0);
        CHECK(partial.texels_real() && !partial.needs_readback(false));
        ok.texels_decoded();                               /* something asked for the 16-byte texels */
        EXPECT(ok, 1, 0, 1, 0, OK, 1, 0);
        ok.used();
        EXPECT(ok, 1, 1, 1, 0, OK, 1, 0);
    }
    {   /* sparse-slab order: the read-back precedes written_compact() */
        NowState s;
        CHECK(s.learned(PN_PARTIAL, true));
        EXPECT(s, 0, 0, 0, 0, PARTIAL, 0, 1);
        s.written_compact();                               /* keeps the knowledge, consumes fresh, texels real */
        EXPECT(s, 1, 0, 1, 0, PARTIAL, 1, 0);
        CHECK(s.texels_real() && !s.host_unknown());
        s.written_compact();                               /* a write without a read-back */
        EXPECT(s, 1, 0, 1, 1, UNKNOWN, 1, 0);
        CHECK(!s.texels_real() && s.host_unknown());
        CHECK(!s.learned(PN_OK, true));                    /* a complete form: no texels */
        EXPECT(s, 1, 0, 1, 1, OK, 1, 1);
        s.written_compact();
        EXPECT(s, 1, 0, 1, 1, OK, 1, 0);
        CHECK(s.learned(PN_REFUSED, true));
        s.written_compact();
        EXPECT(s, 1, 0, 1, 0, REFUSED, 1, 0);
    }
    {   /* a compact form goes stale */
        NowState s = native_compact(PN_OK);
        s.used();
        EXPECT(s, 1, 1, 1, 1, OK, 1, 0);
        CHECK(s.written_texels());                         /* the caller zeroes pal_n on the device ... */
        EXPECT(s, 1, 0, 0, 0, UNKNOWN, 0, 0);
        CHECK(!s.written_texels());                        /* ... exactly once */
        EXPECT(s, 1, 0, 0, 0, UNKNOWN, 0, 0);
        NowState f;                                        /* a pending read-back is dropped by a texel write */
        f.learned(PN_REFUSED, true);
        CHECK(!f.written_texels());
        EXPECT(f, 1, 0, 0, 0, UNKNOWN, 0, 0);
    }
    {   /* replication: a refused source's destinations have real texels */
        const NowState src = native_compact(PN_REFUSED);
        NowState dst = native_compact(PN_OK);
        dst.used();
        CHECK(dst.written_texels());
        dst.adopt(src);
        EXPECT(dst, 1, 0, 1, 0, REFUSED, 1, 0);
        CHECK(dst.texels_real() && !dst.needs_readback(false));
        NowState dst2;                                     /* a complete source: compact form only */
        dst2.written_texels();
        dst2.adopt(native_compact(PN_OK));
        EXPECT(dst2, 1, 0, 1, 1, OK, 1, 0);
        NowState dst3 = native_compact(PN_OK);             /* a source on texels alone */
        NowState tex;
        tex.written_texels();
        tex.used();
        dst3.written_texels();
        dst3.adopt(tex);
        EXPECT(dst3, 1, 0, 0, 0, UNKNOWN, 0, 0);
    }
    {   /* match: the copy into another context */
        NowState partial = native_compact(PN_PARTIAL);
        partial.used(); partial.used();
        NowState d1 = native_compact(PN_OK);
        d1.used();
        d1.adopt_for_match(partial, true, true);
        EXPECT(d1, 1, 0, 1, 0, PARTIAL, 1, 0);
        NowState complete = native_compact(PN_OK);
        complete.used();
        NowState d2;
        d2.learned(PN_REFUSED, true);                      /* whatever the destination held */
        d2.adopt_for_match(complete, false, true);
        EXPECT(d2, 1, 0, 1, 1, OK, 1, 0);
        const NowState sources[3] = {partial, complete, NowState()};
        for (const NowState &src : sources)
            for (int real = 0; real < 2; real++) {
                NowState d3 = native_compact(PN_OK);
                d3.used();
                d3.adopt_for_match(src, real != 0, false);      /* a destination without compact slabs */
                EXPECT(d3, 1, 0, 0, real ? 0 : 1, src.known, src.native, 0);
            }
        NowState unread;                                   /* a compact form the host has not looked at travels as such */
        unread.written_compact();
        NowState d4;
        d4.adopt_for_match(unread, false, true);
        EXPECT(d4, 1, 0, 1, 1, UNKNOWN, 1, 0);
        CHECK(d4.host_unknown());
    }
    {   /* direct compact */
        NowState s = native_compact(PN_OK), plain = native_compact(PN_OK);
        plain.written_texels();
        CHECK(s.written_texels());
        s.direct_compact_written();
        EXPECT(s, 1, 0, 1, 0, UNKNOWN, 0, 0);
        CHECK(s.texels_real() && s.needs_readback(true) && !s.wants_build(false));
        s.direct_compact_refused();
        CHECK(same(s, plain));
        EXPECT(s, 1, 0, 0, 0, UNKNOWN, 0, 0);
    }
    {   /* reset */
        NowState s = native_compact(PN_PARTIAL);
        s.used();
        s.learned(PN_OK, true);
        s.reset();
        CHECK(same(s, NowState()) && !s.ready());
        EXPECT(s, 0, 0, 0, 0, UNKNOWN, 0, 0);
    }
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("now state: ok");
    return 0;
}
