/*
 * dvo_icp_launch.h -- internal interface between the frame-to-model alignment's host code (dvo_capi_icp.cpp) and its kernels
 * (dvo_icp.hip).  Not installed; plain structs only.  The definition is dvo_icp.h.
 */
#ifndef DVO_ICP_LAUNCH_H_
#define DVO_ICP_LAUNCH_H_

#include "dvo_icp.h"

namespace dvo_icp {

constexpr int kLaunchesPerSweep = 2;               /* == DVO_ICP_LAUNCHES_PER_SWEEP: the sweep kernel, the solve kernel */
/* A sweep workgroup has four waves that share its 64 runs, or sixteen when the whole sweep is at most kWideSweepMost workgroups: a
 * short sweep finishes sooner spread over more waves, a long one with fewer waves held at each workgroup's barrier (profiles/icp) */
constexpr int kSweepBlock = 256;
constexpr int kSweepBlockWide = 1024;
constexpr unsigned kWideSweepMost = 512;
constexpr int kSolveBlock = 256;                   /* threads of a solve workgroup */
constexpr int kGroup = 64 * 64;                    /* list entries of one sweep workgroup: two rounds of the tree */
constexpr int kSlots = 32;                         /* rows of a view's partials: the kSums sums, the count (as a double: exact), three unused */
constexpr int kCountSlot = kSums;

/* one view on the device: what the sweeps read, and the state the solve kernel advances (set to the start pose by the upload) */
struct DeviceView {
    View view;
    State state;
};
/* what a view's result is copied back as */
struct DeviceResult {
    double pose12[12];
    dvo_icp_record record;
};
inline unsigned sweep_blocks(int entries) { return (unsigned)((entries + kGroup - 1) / kGroup); }

/* A call's device arrays: views[count]; partials: count * kSlots * stride doubles, row s of view i at (i * kSlots + s) * stride, one
 * entry per sweep workgroup of the view -- stride = sweep_blocks of level 0, the longest list; results[count] */
struct CallArgs {
    DeviceView *views;
    double *partials;
    DeviceResult *results;
    SweepConst c;
    dvo_icp_params p;
    int count;
    unsigned stride;
    bool gated;                                    /* every view has now normals: the sweeps take the gated kernel */
};
/* one sweep of every view that takes part in it: kLaunchesPerSweep launches; record_sweep: the one after level 0.  Returns the hipError_t */
int launch_icp_sweep(const CallArgs &a, int level, bool record_sweep, void *stream);

}  // namespace dvo_icp
#endif
