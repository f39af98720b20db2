/*
 * dvo_now_state.h -- what the HOST knows of one pair's now level: which of its forms (16-byte texels, the compact form of
 * dvo_palette.h) exist and are current.  One record per pair and level (dvo_ctx.h: Level::now), written by the transitions
 * below and by nothing else; each transition says what changed so that its caller (dvo_capi.cpp, dvo_capi_tracker_archive.cpp) can issue
 * the device work that goes with it.  Host only, no HIP header: tests/host/now_state_main.cpp walks it under a sanitizer.
 * Internal; not installed.
 */
#ifndef DVO_NOW_STATE_H_
#define DVO_NOW_STATE_H_

#include "../../include/dvo_amd.h"      /* DVO_COMPACT_NOW_AFTER */

namespace dvo_host {

struct NowState {
    /* what the host knows about the compact form of the current now level -- the device's pal_n says whether the builder (the
     * distance-transform stage, or the generic one) could make it, and the host only learns that where it reads pal_n back: at once
     * on a sparse texel slab (the refused images need memory mapped), otherwise on demand (refresh_compact_known: before a
     * replication and before a launch-shape decision that depends on it).  A REFUSED pair's 16-byte texels are its real form: they
     * are current (texels_stale = 0) and travel with it (round 5, ADVICE r4: a replicated refused source left its destinations
     * without texels -- on a sparse slab without memory behind them). */
    enum : char { P4_UNKNOWN = 0, P4_OK = 1, P4_REFUSED = 2, P4_PARTIAL = 3 /* a partial compact form (dvo_palette.h): read as the compact form, 16-byte texels real too */ };
    static constexpr int PAL_PARTIAL_BIT = 1 << 20;      /* DVO_PAL_PARTIAL of dvo_palette.h (a HIP header); dvo_capi.cpp asserts they agree */

    char present = 0;               /* the now level has been written */
    char built = 0;                 /* the compact form was built from the CURRENT now level (or IS how it was written) */
    /* the now level was written in its compact form only (the engine's own distance-transform stage, round 3) and its 16-byte
     * texels have not been decoded from it yet.  (A pair whose image the compact form could not hold got its texels from the same
     * launch; the decode launch skips it on the device: pal_n <= 0.) */
    char texels_stale = 0;
    char known = P4_UNKNOWN;
    /* set where the engine's own distance-transform stage wrote the compact form (written_compact): such a form is complete or PARTIAL,
     * never refused (dvo_frames.hip) -- what dvo_enqueue's choice of launch shape asks about -- so that choice needs no read-back and
     * no wait on the stream for these pairs (one host sync per level per step of a frames -> align pipeline otherwise) */
    char native = 0;
    char fresh = 0;                 /* learned(.., true) has just read pal_n of the write in flight; consumed by written_compact */
    int uses = 0;                   /* alignments enqueued since the now level was last written */

    /* ---- transitions ---- */
    /* (re)written as 16-byte texels.  Returns true if a current compact form just went stale: the kernel must not read it (the caller
     * zeroes the pair's pal_n on the device) */
    bool written_texels() {
        const bool went_stale = built != 0;
        present = 1; uses = 0; built = 0; texels_stale = 0; known = P4_UNKNOWN; native = 0; fresh = 0;
        return went_stale;
    }
    /* (re)written in the compact form only, by the engine's own distance-transform stage */
    void written_compact() {
        present = 1; uses = 0; built = 1; native = 1;
        if (fresh) fresh = 0;                             /* pal_n of THIS write was read back (sparse slab): known */
        else known = P4_UNKNOWN;
        texels_stale = (known == P4_REFUSED || known == P4_PARTIAL) ? 0 : 1;      /* such an image got its texels from the same launch */
    }
    /* the generic builder ran over the texels; it may have refused (pal_n < 0) */
    void built_compact() { built = 1; known = P4_UNKNOWN; native = 0; }
    /* the host read the device's pal_n; fresh_read: of a write whose written_compact() is still to come.  Returns true if the
     * 16-byte texels are (also) the image's form -- refused, or a partial form: they were written with it */
    bool learned(int pal_n, bool fresh_read) {
        known = pal_n <= 0 ? P4_REFUSED : ((pal_n & PAL_PARTIAL_BIT) ? P4_PARTIAL : P4_OK);
        if (fresh_read) fresh = 1;
        const bool real = known != P4_OK;
        if (real) texels_stale = 0;
        return real;
    }
    void texels_decoded() { texels_stale = 0; }           /* the decode launch wrote the 16-byte texels from the compact form */
    void used() { uses++; }                               /* one more alignment enqueued */
    /* dvo_set_now_level's direct route, after written_texels(): texels AND compact form are current, pal_n on the device says which
     * one the kernel reads; refused: not an exact distance transform, the pair is left to the generic builder's policy */
    void direct_compact_written() { built = 1; }
    void direct_compact_refused() { built = 0; }
    /* the destination of a device-side copy of src's now level, in the form(s) src has */
    void adopt(const NowState &src) {
        present = 1; uses = 0; fresh = 0;
        built = src.built; texels_stale = src.texels_stale; known = src.known; native = src.native;
    }
    /* ... into another context (dvo_tracker_match): texels_real = the copy wrote real 16-byte texels, as far as the host knows;
     * a destination without the compact form's slabs has no compact form whatever the source has */
    void adopt_for_match(const NowState &src, bool texels_real, bool dst_has_compact_slabs) {
        adopt(src);
        if (!dst_has_compact_slabs) built = 0;
        texels_stale = texels_real ? 0 : 1;
    }
    void reset() { *this = NowState(); }

    /* ---- queries ---- */
    bool ready() const { return present != 0; }
    bool texels_real() const { return !texels_stale; }
    /* the generic builder should run: with only_reused, only once the level has been aligned DVO_COMPACT_NOW_AFTER times */
    bool wants_build(bool only_reused) const { return present && !built && (!only_reused || uses >= DVO_COMPACT_NOW_AFTER); }
    /* pal_n is worth reading back (skip_native: only where a refusal is possible) */
    bool needs_readback(bool skip_native) const { return built && known == P4_UNKNOWN && !(skip_native && native); }
    bool host_unknown() const { return needs_readback(false); }      /* a compact form the host has not looked at */
};

}  // namespace dvo_host
#endif
