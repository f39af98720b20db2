/*
 * multi_track_demo.cpp -- track_demo for N sequences at once on dvo_amd::SolveDVOStreams: reads <dir_s>/framemono_%04d.xml of
 * every stream s (OpenCV FileStorage XML, mono_0.. / depth_0..), advances all streams that still have a frame by one frame per
 * tick, and writes one "qx qy qz qw tx ty tz" line per frame after the first (printPose, SolveDVO.cpp:1341-1354) to
 * <out_prefix><s>.txt -- per stream the file track_demo writes for that sequence alone.
 *
 *   multi_track_demo <n_streams> <dir_0> .. <dir_n-1> <start> <end> <skip> <n_levels> <fx> <fy> <cx> <cy> <iters_per_level> <out_prefix>
 *                    [<laplacian_b_thresh> <visible_ratio_thresh> <min_points>]     the reference's adaptive key-frame exits (:2129-2152)
 *                    [--sigma]      last argument: also print, per pose, the six standard deviations of its covariance
 *                                   (dvo_amd::poseCovariance of the tracker's information matrix; translation x y z, rotation x y z)
 *                    [--views DIR]  trailing option: also write stream 0's two views of every frame (the reprojections on the distance
 *                                   transform, the residue heat map) to DIR/reproj_%04ld.ppm and DIR/heat_%04ld.ppm (binary PPM)
 *                    [--places K]   trailing option: keep the key frames in an archive of 256 slots with place descriptors of the
 *                                   coarsest level and, every tick, query the K nearest archived key frames of every stream's current
 *                                   frame, align each stream against its top candidate and print one line per stream; then verify
 *                                   each aligned candidate against the current frame's depth and print its record and verdict
 *                    [--shift R]    trailing option, with --places: register every one of the K candidates on the stream's current frame
 *                                   by a shift search of radius R on the descriptors (R is cut to what the coarsest level allows), take
 *                                   per stream the candidate with the smallest best-shift SAD instead of the top one, print its shift
 *                                   record, and start its alignment from the rotation guess of that shift instead of the identity
 *                    [--mask-bottom N]  trailing option: ignore the lowest N rows of every stream's frames (a bonnet, a bumper): one
 *                                   ignore mask for all streams (SolveDVOStreams::setStreamMask, margin 2), in rows of level 0
 *                    [--save-archive FILE]  trailing option: keep the key frames in the archive (as --places does) and write them all to
 *                                   FILE when the run ends (SolveDVOStreams::saveArchive: "save map")
 *                    [--load-archive FILE]  trailing option: before the first frame, take the key frames of FILE into the archive ("load
 *                                   map"); with --places the streams are then relocalised against them from their first frame on -- a
 *                                   loaded key frame is printed with stream -1 and the frame number it had in the run that saved it
 */
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>

#include "dvo_amd.hpp"

int main(int argc, char **argv) {
    bool sigma = false;
    std::string views_dir;
    int places_k = 0, shift_r = -1, mask_bottom = 0;
    std::string save_archive, load_archive;
    for (bool more = true; more;) {                          /* trailing options, in any order */
        more = false;
        if (argc > 2 && std::string(argv[argc - 1]) == "--sigma") { sigma = true; argc--; more = true; }
        if (argc > 3 && std::string(argv[argc - 2]) == "--views") { views_dir = argv[argc - 1]; argc -= 2; more = true; }
        if (argc > 3 && std::string(argv[argc - 2]) == "--places") { places_k = std::atoi(argv[argc - 1]); argc -= 2; more = true; }
        if (argc > 3 && std::string(argv[argc - 2]) == "--shift") { shift_r = std::atoi(argv[argc - 1]); argc -= 2; more = true; }
        if (argc > 3 && std::string(argv[argc - 2]) == "--mask-bottom") { mask_bottom = std::atoi(argv[argc - 1]); argc -= 2; more = true; }
        if (argc > 3 && std::string(argv[argc - 2]) == "--save-archive") { save_archive = argv[argc - 1]; argc -= 2; more = true; }
        if (argc > 3 && std::string(argv[argc - 2]) == "--load-archive") { load_archive = argv[argc - 1]; argc -= 2; more = true; }
    }
    const int ns = argc > 1 ? std::atoi(argv[1]) : 0;
    const int base = 2 + ns;
    if (ns < 1 || (argc != base + 10 && argc != base + 13)) {
        std::fprintf(stderr, "usage: %s n_streams dir_0 .. dir_n-1 start end skip n_levels fx fy cx cy iters out_prefix "
                             "[laplacian_b_thresh visible_ratio_thresh min_points] [--sigma] [--views DIR] [--places K] [--shift R] [--mask-bottom N] "
                             "[--save-archive FILE] [--load-archive FILE]\n", argv[0]);
        return 2;
    }
    const int start = std::atoi(argv[base]), end = std::atoi(argv[base + 1]), skip = std::atoi(argv[base + 2]), nl = std::atoi(argv[base + 3]);
    const int iters = std::atoi(argv[base + 8]);
    const std::string prefix = argv[base + 9];
    try {
        /* the first stream's first frame gives the geometry of every stream */
        char name[1024];
        std::string text;
        std::vector<double> v, w;
        dvo_amd::RGBDFramePyd probe;
        std::snprintf(name, sizeof(name), "%s/framemono_%04d.xml", argv[2], start);
        if (!dvo_amd::loadFrameXml(name, nl, probe, text, v, w)) { std::fprintf(stderr, "cannot read %s\n", name); return 1; }
        dvo_tracker_params tp;
        dvo_tracker_params_default(&tp);
        tp.rows = probe.levels[0].rows; tp.cols = probe.levels[0].cols; tp.n_levels = nl; tp.first_shift = 0;
        for (int l = 0; l < DVO_MAX_LEVELS; l++) tp.iters[l] = l < nl ? iters : 0;
        if (argc == base + 13) {
            tp.adaptive = 1;
            tp.laplacian_b_thresh = (float)std::atof(argv[base + 10]);
            tp.visible_ratio_thresh = (float)std::atof(argv[base + 11]);
            tp.min_points = std::atoi(argv[base + 12]);
        }
        dvo_amd::SolveDVOStreams dvo(ns, &tp);
        if (sigma) dvo.enableInformation();
        if (!views_dir.empty()) dvo.enableViews();
        if (places_k > 0 || !save_archive.empty() || !load_archive.empty()) { dvo.enableArchive(256, ns); dvo.enablePlaces(nl - 1); }
        if (mask_bottom > 0) {                               /* the frames arrive as pyramids: the mask is given at level 0's size */
            std::vector<unsigned char> mask((size_t)tp.rows * tp.cols, 0);
            const int first = tp.rows - std::min(mask_bottom, tp.rows);
            std::fill(mask.begin() + (size_t)first * tp.cols, mask.end(), (unsigned char)255);
            dvo.setStreamMask(-1, mask.data());
        }
        if (shift_r > DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS) shift_r = DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS;
        while (shift_r > 0 && (probe.levels[nl - 1].rows - 2 * shift_r < 1 || probe.levels[nl - 1].cols - 2 * shift_r < 1)) shift_r--;
        dvo.setCameraMatrix((float)std::atof(argv[base + 4]), (float)std::atof(argv[base + 5]), (float)std::atof(argv[base + 6]),
                            (float)std::atof(argv[base + 7]));
        if (!load_archive.empty()) {
            const std::vector<long long> ids = dvo.loadArchive(load_archive);
            std::printf("loaded %zu key frames from %s:", ids.size(), load_archive.c_str());
            for (long long id : ids) std::printf(" %lld", id);
            std::printf("\n");
        }
        std::vector<std::unique_ptr<std::ofstream>> poses;
        for (int s = 0; s < ns; s++) poses.emplace_back(new std::ofstream(prefix + std::to_string(s) + ".txt"));
        std::vector<dvo_amd::RGBDFramePyd> frames(ns);
        std::vector<char> live(ns, 1);
        double step_ms = 0;
        long ticks = 0, tracked = 0;
        for (long n = 0;; n++) {
            const int idx = start + skip * (int)n;
            if (idx > end) break;
            std::vector<int> streams;
            std::vector<const dvo_amd::RGBDFramePyd *> fp;
            for (int s = 0; s < ns; s++) {
                if (!live[s]) continue;
                std::snprintf(name, sizeof(name), "%s/framemono_%04d.xml", argv[2 + s], idx);
                if (!dvo_amd::loadFrameXml(name, nl, frames[s], text, v, w)) { live[s] = 0; continue; }    /* that sequence has ended */
                streams.push_back(s);
                fp.push_back(&frames[s]);
            }
            if (streams.empty()) break;
            const auto t0 = std::chrono::steady_clock::now();
            const std::vector<dvo_amd::Pose> p = dvo.processFrames(streams, fp);
            step_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            ticks++;
            if (!views_dir.empty() && streams[0] == 0)
                for (int which : {DVO_VIEW_REPROJ_ON_DT, DVO_VIEW_RESIDUE_HEAT}) {
                    const dvo_amd::SolveDVOStreams::View im = dvo.lastView(0, which);
                    std::snprintf(name, sizeof(name), "%s/%s_%04ld.ppm", views_dir.c_str(), which == DVO_VIEW_REPROJ_ON_DT ? "reproj" : "heat", n);
                    std::ofstream f(name, std::ios::binary);
                    f << "P6\n" << im.cols << " " << im.rows << "\n255\n";
                    for (size_t k = 0; k + 2 < im.bgr.size(); k += 3) f << im.bgr[k + 2] << im.bgr[k + 1] << im.bgr[k];      /* PPM is R G B */
                }
            if (places_k > 0) {                                        /* candidates -> match: frames at least 10 apart on the same stream */
                const std::vector<std::vector<dvo_tracker_place>> found = dvo.queryPlaces(streams, places_k, 10);
                std::vector<dvo_amd::SolveDVOStreams::Candidate> cand;
                std::vector<size_t> chosen(streams.size(), 0);         /* per stream: which of its candidates is aligned */
                if (shift_r >= 0) {                                    /* query -> shifts -> guess -> match -> verify */
                    std::vector<int> cs;
                    std::vector<long long> ck;
                    for (size_t i = 0; i < streams.size(); i++)
                        for (const dvo_tracker_place &pl : found[i]) { cs.push_back(streams[i]); ck.push_back(pl.key_id); }
                    std::vector<dvo_tracker_place_shift> sh;
                    if (!cs.empty()) sh = dvo.placeShifts(cs, ck, shift_r);
                    size_t at = 0;
                    for (size_t i = 0; i < streams.size(); at += found[i].size(), i++) {
                        if (found[i].empty()) continue;
                        for (size_t j = 1; j < found[i].size(); j++)
                            if (sh[at + j].sad < sh[at + chosen[i]].sad) chosen[i] = j;
                        const dvo_tracker_place_shift &b = sh[at + chosen[i]];
                        cand.emplace_back();
                        cand.back().stream = streams[i]; cand.back().keyId = found[i][chosen[i]].key_id;
                        dvo.placeGuess(cand.back(), b);
                        std::printf("stream %d frame %ld shift key %lld dy %d dx %d sad %u zero %u second %u area %d\n", streams[i], n,
                                    cand.back().keyId, b.dy, b.dx, b.sad, b.sad_zero, b.sad_second, b.area);
                    }
                } else {
                    for (size_t i = 0; i < streams.size(); i++)
                        if (!found[i].empty()) { cand.emplace_back(); cand.back().stream = streams[i]; cand.back().keyId = found[i][0].key_id; }
                }
                if (!cand.empty()) dvo.matchKeyFrames(cand);
                /* the independent check of each aligned candidate: its key frame's points against the current frame's DEPTH, at the pose
                 * the match returned, on the finest level */
                std::vector<dvo_tracker_verify_record> ver;
                if (!cand.empty()) ver = dvo.verifyKeyFrames(cand, 0);
                for (size_t k = 0; k < ver.size(); k++)
                    std::printf("stream %d frame %ld verify key %lld points %d visible %d depth %d agree %d front %d behind %d sum_abs_q4 %llu "
                                "verdict %d\n", cand[k].stream, n, cand[k].keyId, ver[k].n_points, ver[k].n_visible, ver[k].n_depth, ver[k].n_agree,
                                ver[k].n_front, ver[k].n_behind, ver[k].sum_abs_q4, dvo_amd::depthVerdict(ver[k], 0.8, 0.05, 100) ? 1 : 0);
                size_t c = 0;
                for (size_t i = 0; i < streams.size(); i++) {
                    if (found[i].empty()) { std::printf("stream %d frame %ld place none\n", streams[i], n); continue; }
                    const dvo_tracker_place &pl = found[i][chosen[i]];
                    const dvo_tracker_score_record &r = cand[c++].rec;
                    std::printf("stream %d frame %ld place key %lld (stream %d frame %lld) distance %u visible %d of %d\n", streams[i], n,
                                pl.key_id, pl.stream, pl.frame, pl.distance, r.n_visible, r.n_points);
                }
            }
            for (size_t i = 0; i < streams.size(); i++) {
                if (dvo.lastEvents[i] == 1) continue;                  /* no pose line for a first frame, like the reference */
                dvo_amd::SolveDVO::printPose(p[i], *poses[streams[i]]);
                if (sigma) {
                    const dvo_amd::SolveDVOStreams::Information r = dvo.lastInformation(streams[i]);
                    double C[36];
                    if (dvo_amd::poseCovariance(r.H, r.sum_eps2, r.n_visible, C))
                        std::printf("stream %d frame %ld sigma %.6g %.6g %.6g %.6g %.6g %.6g\n", streams[i], n, std::sqrt(C[0]), std::sqrt(C[7]),
                                    std::sqrt(C[14]), std::sqrt(C[21]), std::sqrt(C[28]), std::sqrt(C[35]));
                    else
                        std::printf("stream %d frame %ld sigma none (%d visible points)\n", streams[i], n, r.n_visible);
                }
                tracked++;
            }
        }
        for (int s = 0; s < ns; s++) {
            const dvo_amd::GOP<double> &g = dvo.gop[s];
            std::printf("stream %d frames %d keyframes:", s, g.size());
            for (int i = 0; i < g.size(); i++) if (g.isKeyFrameAt(i)) std::printf(" %d(reason %d)", g.getFrameNumAt(i), g.getReasonAt(i));
            std::printf("\n");
        }
        if (ticks) std::printf("ticks %ld, %.3f ms per tick, %ld poses\n", ticks, step_ms / ticks, tracked);
        if (!save_archive.empty()) {
            dvo.saveArchive(save_archive);
            std::printf("saved the archive to %s\n", save_archive.c_str());
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "multi_track_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
